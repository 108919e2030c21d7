/*
 * t4k.h - C-ABI of the MI355X (gfx950) tensor/CNN kernel backend for tensorForth.
 *
 * This is the drop-in boundary: every entry point below replaces one CUDA kernel
 * (or one host wrapper + kernel pair) of the reference, cited as file:line
 * relative to the reference tree.  All pointers are plain device pointers
 * (fp32 unless noted), all sizes plain ints/longs; no C++ / torch types.
 *
 * Conventions (reference src/mu/tensor.h:51-115):
 *   - tensors are fp32, NHWC contiguous; a sample slice is data + n*H*W*C
 *   - every call returns an int status (T4K_OK == 0); nothing throws or aborts
 *     (reference convention is print-and-continue, src/ten4_types.h:25,186-191)
 *   - calls are asynchronous on `stream` (NULL = the library's default stream);
 *     the caller synchronises (t4k_sync) before touching results on the host.
 *     The reference syncs after every launch (GPU_CHK, src/ten4_types.h:192);
 *     here the host layer syncs only at the host-touch sites.
 *   - kernels never allocate; scratch comes from a library-owned workspace that
 *     replaces the reference's per-tensor `_tmp` slot (src/mu/tensor.cu:481).
 */
#ifndef T4K_H_
#define T4K_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *t4k_stream_t;            /* hipStream_t */
typedef void *t4k_event_t;             /* hipEvent_t  */
typedef void *t4k_graph_t;             /* hipGraphExec_t */

enum {
    T4K_OK              =  0,
    T4K_ERR_ARG         = -1,          /* bad shape / null pointer / unsupported parameter   */
    T4K_ERR_HIP         = -2,          /* HIP runtime error (see t4k_last_error)             */
    T4K_ERR_NOMEM       = -3,
    T4K_ERR_UNSUPPORTED = -4,          /* e.g. conv (K,S,P) outside the reference's set      */
    T4K_ERR_NODEVICE    = -5,          /* no gfx950 device: the product path fails loudly    */
    T4K_ERR_SINGULAR    = -6           /* singular matrix in inverse/plu                     */
};

/* math_op: values identical to reference src/t4math.h:25-56 */
enum {
    T4K_ABS = 0, T4K_NEG, T4K_EXP, T4K_LN, T4K_LOG, T4K_TANH, T4K_RELU, T4K_SIGM,
    T4K_SQRT, T4K_RCP, T4K_SAT, T4K_IDEN, T4K_FILL, T4K_GFILL, T4K_SCALE, T4K_POW,
    T4K_ADD, T4K_SUB, T4K_MUL, T4K_DIV, T4K_MOD, T4K_MAX, T4K_MIN, T4K_MUL2, T4K_MOD2,
    T4K_SIN, T4K_COS
};
/* t4_layer: values identical to reference src/nn/ntypes.h:16-36 */
enum {
    T4K_L_NONE = 0, T4K_L_CONV, T4K_L_LINEAR, T4K_L_FLATTEN, T4K_L_RELU, T4K_L_TANH,
    T4K_L_SIGMOID, T4K_L_SELU, T4K_L_LEAKYRL, T4K_L_ELU, T4K_L_DROPOUT, T4K_L_SOFTMAX,
    T4K_L_LOGSMAX, T4K_L_AVGPOOL, T4K_L_MAXPOOL, T4K_L_MINPOOL, T4K_L_BATCHNM,
    T4K_L_USAMPLE, T4K_L_DCONV,
    T4K_L_ATTN,                        /* beyond the reference's list (appended, no value moves): multi-head attention, `vector{ heads causal } linear` */
    T4K_L_ADDNORM,                     /* ... and add & norm, out = norm(x + skip), `vector{ back mode } selu` */
    T4K_L_EMBED                        /* ... and the embedding layer, token and learned position tables, `vector{ V E pos } upsample` */
};
/* rand_opt: reference src/util.h:22-25 */
enum { T4K_UNIFORM = 0, T4K_NORMAL = 1 };
/* reduction selector for t4k_reduce */
enum { T4K_RED_SUM = 0, T4K_RED_NVAR, T4K_RED_MAX, T4K_RED_MIN };

/* ------------------------------------------------------------------ runtime */
/* Replaces cudaSetDevice / cudaMallocManaged arena / cudaMemcpy / cudaDeviceSynchronize
 * uses (src/ten4.cu:125-152, src/mu/mmu.cu:44-46, src/ten4_types.h:192-201). */
int         t4k_device_count(void);
int         t4k_init(int device);                  /* select device, create default stream + workspace */
void        t4k_shutdown(void);
/* Kernels whose workgroups wait for each other (arrival gates of the one-launch dW || dX products, pair-mode tickets, the band exchange of the conv-stack
 * head, column-stripe tickets) need every workgroup of the launch resident at once: true on an exclusively owned device, not on a partitioned or shared
 * one.  t4k_gates_enable(0) makes every launcher pick its ungated path (more launches, same results); a wait that times out does it by itself, after
 * reporting T4K_ERR_HIP once for the launch it spoiled (runtime.hip spin_check). */
int t4k_gates_enable(int on);
int t4k_gates_enabled(void);
const char *t4k_last_error(void);
const char *t4k_backend_name(void);                /* "hip-gfx950" for the product library */
int         t4k_device_info(int *cu_count, int *clock_khz, size_t *hbm_bytes);

int t4k_malloc(void **p, size_t bytes);            /* device (HBM) allocation */
int t4k_free(void *p);
int t4k_host_alloc(void **p, size_t bytes);        /* pinned host staging */
int t4k_host_free(void *p);
int t4k_memcpy_h2d(void *dst, const void *src, size_t bytes, t4k_stream_t s);
int t4k_memcpy_d2h(void *dst, const void *src, size_t bytes, t4k_stream_t s);
int t4k_memcpy_d2d(void *dst, const void *src, size_t bytes, t4k_stream_t s);
int t4k_memset(void *dst, int byte, size_t bytes, t4k_stream_t s);   /* Tensor::zeros tensor.cu:558-563 */
int t4k_sync(t4k_stream_t s);
/* Kernels launched by the library since t4k_init (every launch site counts itself): measurement hook - bench.py brackets its timed
 * loop with it and prints the MEASURED launches per step (the reference issues one launch + cudaDeviceSynchronize per layer,
 * src/nn/forward.cu:82-113, backprop.cu:111-140; memcpy / memset / collective commands are not kernels and are not counted). */
unsigned long long t4k_launch_count(void);
/* The rung of the GEMM dispatch ladder (csrc/gemm.hip gemm_launch) the last product of this process took, as a static string: test hook - the
 * GEMM sweep asserts it for every shape of its table.  "l32/w8/rst", "pair", "nn_plain", "plain_any", "plain_ragk", "plain128", "plain128/ragk",
 * "plain128/bk32", "plain256", "glds8<128>", "glds8<64,ragk>", "mfma<128,128,32,vec,full>", "mfma<64,64,64,vec,skew>", "mfma<64,64,32>", "k0"
 * (K = 0: O = beta O), "none" (M or N = 0); "xN" behind it for N split-K slabs and "+fold" when the fold launch followed them.  Valid until the
 * next call of this function.  gemm_launch keeps the rung, N and the fold of the plan it ran in one plain, unsynchronised store: read it on the thread
 * that issued the product, right behind the call - a product issued from a second host thread, or a later entry that reaches gemm_launch, overwrites it. */
const char *t4k_gemm_last_plan(void);
/* The plan gemm_launch makes for one product, on the host alone: the same planner (csrc/gemm.hip gemm_plan), nothing launched, no device and no
 * t4k_init needed.  flags says what the planner cannot see from the extents: */
enum { T4K_GP_A16 = 1, T4K_GP_B16 = 2,   /* A, B on 16 bytes */
       T4K_GP_EPILOGUE = 4,              /* (alpha, beta) != (1, 0) */
       T4K_GP_BIAS = 8,                  /* a bias row */
       T4K_GP_RIDER = 16,                /* an activation epilogue or a rider of the last launch is asked for (the linear layers) */
       T4K_GP_DEFER = 32,                /* the caller folds split-K slabs itself (t4k_mlp_head_fwd) */
       T4K_GP_LANE = 64,                 /* a stream other than the default one */
       T4K_GP_CAPTURING = 128,           /* the stream is being captured into a graph */
       T4K_GP_GATES_OFF = 256 };         /* t4k_gates_enable(0) */
/* cs_rows != 0: a column-sum request over that many rows (the bias gradient offered to a weight-gradient product); cu: the CU count to plan for, 0 = the
 * library's current one (256 before t4k_init); ws_bytes: the stream's workspace, 0 = the library's (64 MiB).  The zero block and the tickets of an
 * initialised library are taken as present.
 * text: what t4k_gemm_last_plan() reports after that call, byte for byte;
 * out = { split-K slabs, K depth of a slab (of a sliver workgroup; K itself on the lean kernels; 0 for "none" and "k0"), kernel launches,
 *         a rider would ride (in the product's launch or in its fold), the column sums ride, the slabs are left to the caller }.
 * NULL text or out, cu < 0 or ws_bytes < 0: T4K_ERR_ARG; a negative extent or C < 1: T4K_ERR_ARG as t4k_gemm. */
int t4k_gemm_plan(int M, int N, int K, int C, int tA, int tB, unsigned flags, int cs_rows, int cu, long ws_bytes, char text[64], int out[6]);
/* The engine decisions of the last convolution entry of this process (t4k_conv2d_fwd / _fwd2 / _bn_fwd / _bn_block_fwd / _block_fwd / _bwd / _bwd2,
 * t4k_dconv2d_fwd / _bwd), in launch order, as one static string of blank-separated tokens: test hook - the conv sweep asserts it for every row
 * of its table.  Forward: "few<G,CH,VW>", "thin" ("+copy": the layer-0 copy leaves from the same launch, "+stat": the batch-norm sums ride),
 * "img_block", "gather<raw|staged,ksN>", "gather_pool<raw|staged,ksN>", "big<64|128>", "big8<64|128,bk64|bk32>" ("+bn": the batch-norm rider);
 * "memcpy": the layer-0 copy was a copy command.  dF | dB: "dfw<ciw,ntw>xN", "df8<tp1|tp2>xN", "dfxN" (N slices; no bias row: dB is "colsum<chunks>",
 * "+fold" behind it when the chunks are folded by a second launch), "thin_dfxN+b", "df_mfmaxN+b" ("+b": the bias row of the slab is dB); the fold of
 * the slices: "fold_add" or "df_fold" as launches of their own, or "+fold" behind the dX engine that carries it.  dX: "dx_big8<..>", "dx_big<..>",
 * "dx_wide<lanes per pixel>", "dx_few", "fewch<G,CH,VW>", "dx_and_fold<raw|staged,ksN>".  The transposed convolution adds "xpose" per filter
 * transposition and "bias".  The run-time-geometry entries (t4k_conv2d_geo_fwd / _bwd): "geo<64|128,v4|v1,f4|f1>" (channel tile, 16-byte or dword
 * gather, 16-byte or dword filter loads), "geo_dfxN<tap|rows,d4|rows,d1>" (N slices, the bias row in the slab; a tile's rows one tap's channels, or (c1, tap) rows with 16-byte / dword dO), "fold_add" or "df_fold", "geo_dx<64|128,v4|v1>".  The grouped entries (t4k_conv2d_grp_fwd / _bwd): "grp_dw<v4|v1>" (depthwise, Cg1 == 1) or "grp<v4|v1>" (4 output
 * channels per thread with 16-byte loads and stores, or one with dwords), "grp_dfxN" (N slices, the bias row in the slab), "fold_add" or "df_fold", "grp_dx<v4|v1>".  Valid until the next call of this function; plain, unsynchronised stores as t4k_gemm_last_plan. */
const char *t4k_conv_last_plan(void);

/* Library streams own a private workspace, so independent work (e.g. dW beside dX) may be forked
 * onto them and still be captured into one graph through event edges. */
int t4k_stream_create(t4k_stream_t *s);
/* A stream WITHOUT a library workspace: copies and element-wise launches only (the batch prefetch of the dataset feed,
 * src/mu/dataset.cu:112 "TODO: async prefetch"); not a lane - kernels that need split-K / partial slabs refuse or serialise on it. */
int t4k_stream_create_plain(t4k_stream_t *s);
int t4k_stream_destroy(t4k_stream_t s);
int t4k_stream_wait_event(t4k_stream_t s, t4k_event_t e);   /* fork / join edge (also inside a capture) */
int t4k_set_default_stream(t4k_stream_t s);        /* adopt an external stream (e.g. torch's current) */
t4k_stream_t t4k_default_stream(void);

int t4k_event_create(t4k_event_t *e);
int t4k_event_record(t4k_event_t e, t4k_stream_t s);
int t4k_event_sync(t4k_event_t e);
/* the wait of a helper thread (host/dataset.cpp's reader): only the wait - no deferred work of the model's thread is run, the wait-error word is left alone */
int t4k_event_wait(t4k_event_t e);
int t4k_event_elapsed_ms(t4k_event_t start, t4k_event_t stop, float *ms);
int t4k_event_destroy(t4k_event_t e);

/* ---------------------------------------------------------------- data-parallel exchange
 * One process per GPU.  Rank 0 makes a 128-byte id, the launcher hands it to every rank (any side channel), each
 * rank joins; afterwards t4k_allreduce_sum() sums a device buffer in place over all ranks on the given stream
 * (RCCL over xGMI).  The host VM calls it on the model's gradient slab between `backprop` and the optimizer. */
int t4k_comm_unique_id(void *id128);
int t4k_comm_init(const void *id128, int rank, int world);
int t4k_comm_world(void);                          /* 0 = no communicator */
int t4k_comm_rank(void);
int t4k_allreduce_sum(float *buf, long n, t4k_stream_t s);
int t4k_comm_destroy(void);
/* Batch-norm statistics over the WHOLE batch (all ranks) instead of the rank's shard: off by default.  When on, every
 * t4k_batchnorm_fwd / _bwd issues one [2C] all-reduce, so EVERY rank must make the same batch-norm calls in the same order - the host
 * switches it on for training passes only (an evaluation pass that only some ranks run would hang in the collective). */
int t4k_comm_sync_batchnorm(int on);

/* ONE-SHOT gradient exchange over peer-mapped windows (csrc/xchg.hip; the reference has no multi-GPU path - the seam is Model::sgd / adam,
 * src/nn/gradient.cu:63-142).  Every rank allocates a receive window (t4k_xchg_create -> a 64-byte IPC handle), the launcher hands all
 * handles to all ranks, every rank maps its peers (t4k_xchg_connect).  From then on t4k_opt_step_dp() sums the gradient slab over all ranks
 * INSIDE the optimizer launch: each rank writes {epoch, value} words straight into every peer's window (xGMI is point to point: all links
 * at once) and adds the `world` copies of each element in rank order - fold + all-reduce + update in one launch, no collective kernel.
 * t4k_comm_world / t4k_comm_rank report the exchange's job when no RCCL communicator exists, and t4k_allreduce_sum then sums over the same
 * windows, so the host's scalar reductions need no second transport.  Dropout masks are keyed by the sample's place in the whole batch
 * from t4k_xchg_connect on (as after t4k_comm_init).  Waits for a peer are bounded: a missing rank gives T4K_ERR_HIP at the next t4k_sync. */
int t4k_xchg_create(long slab_floats, int rank, int world, void *handle64);
int t4k_xchg_connect(const void *handles /* world x 64 bytes, rank order */);
int t4k_xchg_allreduce(float *buf, long n, t4k_stream_t s);   /* in-place SUM over the ranks through the windows (any n; rank order: deterministic) */
int t4k_xchg_trust(int on);                        /* the launcher's verdict on the known-sum probe (tensorforth_amd/dp.py): waits are bounded by 2 s until it is 1, by T4K_XCHG_TIMEOUT_MS (20 s) after */
int t4k_xchg_self(int on);                         /* measurement: a one-rank job takes the exchanging optimizer launch too (bench.py dp_overhead_us) */
int t4k_xchg_active(void);                         /* 1 when t4k_opt_step_dp will exchange (connected and world > 1, or self mode) */
int t4k_xchg_world(void);                          /* 0 = not connected */
int t4k_xchg_rank(void);
int t4k_xchg_destroy(void);

/* hipGraph capture of a launch sequence (replaces ~40 launch+sync pairs per training
 * step of the reference).  begin..end captures every t4k_* kernel call
 * issued on `s`; launch replays it. */
int t4k_graph_begin(t4k_stream_t s);
int t4k_graph_end(t4k_stream_t s, t4k_graph_t *g);
int t4k_graph_launch(t4k_graph_t g, t4k_stream_t s);
int t4k_graph_destroy(t4k_graph_t g);

/* ------------------------------------------------- tensor kernels (t4math.cu) */
/* k_sum :23, k_nvar :48, k_max/d__max :85-131 via Tensor::sum/std/norm/max/min
 * (tensor.cu:224-277).  Result is written (not accumulated) to *out_dev. */
int t4k_reduce(int red_op, const float *src, long n, float avg, float *out_dev, t4k_stream_t s);
/* The same reductions along any subset of the axes, NumPy keepdims=True; no reference definition: k_sum :23, k_nvar :48 and
 * k_max :85-131 fold a whole tensor into one scalar, and the reference's only axis reductions are parts of nn layers (k_dlinear_db
 * nmath.cu:274, k_batchnorm_1 nmath.cu:177, the softmax row sum forward.cu:222-243).
 *   src is dense NHWC of extents dim = {N,H,W,C}; mask adds N = 8, H = 4, W = 2, C = 1 for the axes folded; dst is dense NHWC with
 *   every masked axis at extent 1.  red_op as t4k_reduce (SUM: sum x, NVAR: sum (x - c)^2, MAX, MIN); center is read for NVAR only,
 *   laid out as dst: the value c subtracted for that output (NULL: 0).  A masked axis of extent 1 has no effect.
 * One launch, or two when few outputs stand behind long reductions (partials in the stream's workspace, folded in index order);
 * no allocation, no synchronisation, no floating-point atomics: the same bits on every run.
 * NULL src / dst / dim, an extent < 1, a mask outside 1..15, an unknown red_op, more than 2^40 elements or dst overlapping src:
 * T4K_ERR_ARG. */
int t4k_reduce_axes(int red_op, const float *src, float *dst, const int dim[4], int mask,
                    const float *center, t4k_stream_t s);
/* The plan t4k_reduce_axes takes for (dim, mask) when src is (aligned != 0) or is not 16-byte aligned; launches nothing.  ws_bytes > 0
 * plans for a workspace of that size and needs no device and no t4k_init; ws_bytes == 0 means the initialised library's own workspace
 * (T4K_ERR_NODEVICE before t4k_init); ws_bytes < 0 or NULL out: T4K_ERR_ARG, and dim / mask as t4k_reduce_axes.
 * out = { family (0 row: innermost group reduced, 1 column), launches, float4 path (0 / 1),
 *         row: log2 of the lanes of a group | column: log2 of a tile's lanes,
 *         row: log2 of the lanes side by side along a run | column: tiles along the kept extent,
 *         parts per group, the extent dealt to the parts (0 none; 1 the units of a run (row) or the rows (column); 2 the outer reduced
 *         extent), passes of the grid-stride loop = ceil(work items / 2048) }.
 * With two launches this is the first; the second is the same planner applied to the partials (S floats behind each output). */
int t4k_reduce_axes_plan(const int dim[4], int mask, int aligned, long ws_bytes, int out[8]);
/* Softmax along any subset of the axes: for every index of the unmasked axes the elements along the masked axes form one group,
 * x <- exp(x - max_group) / sum_group exp(x - max_group).  No reference definition: the reference's only softmax forms are the layer's
 * rows (_fsoftmax forward.cu:222-243, t4k_softmax below) and the whole-tensor word (netvm.cpp:36-39).
 *   src and dst are dense NHWC of extents dim = {N,H,W,C}; mask adds N = 8, H = 4, W = 2, C = 1 for the axes of a group.  dst == src is
 *   allowed (in place).  A masked axis of extent 1 has no effect; a group of one element becomes 1.
 * Arithmetic as t4k_softmax: max shift, __expf, fp32 sum, one fp32 division per element.  Inputs are finite, with one exception: -inf is
 * admitted where the group keeps a finite element (the masking idiom) - such an element becomes exactly +0 in every regime and takes no
 * part in the others' values.  The result for +inf, NaN or a group of nothing but -inf is unspecified.
 * One launch while a lane's share of a group fits its registers, or as two passes over the source inside one launch (a running
 * (max, sum) pair, rescaled when the max moves); for few groups behind long reductions three launches: parts of a group leave pairs in
 * the stream's workspace, a merge folds them in index order, a last launch normalises.  No allocation, no synchronisation, no read-back,
 * no floating-point atomics: the same bits on every run; legal under graph capture.
 * NULL src / dst / dim, an extent < 1, a mask outside 1..15, more than 2^40 elements, or dst overlapping src other than dst == src:
 * T4K_ERR_ARG. */
int t4k_softmax_axes(const float *src, float *dst, const int dim[4], int mask, t4k_stream_t s);
/* The plan t4k_softmax_axes takes for (dim, mask) when both pointers are (aligned != 0) or are not 16-byte aligned; launches nothing.
 * out = { family (0 row: innermost group reduced, 1 column), regime (0 registers, 1 two passes in one launch, 2 three launches),
 *         float4 path (0 / 1), log2 of the lanes of a group (row) or of a tile's lanes (column), parts per group,
 *         rescales of the running sum on an element's way into its group's sum (0 in regime 0) }. */
int t4k_softmax_axes_plan(const int dim[4], int mask, int aligned, int out[6]);
/* The launch geometry behind that plan: out[8] and ws_bytes as t4k_reduce_axes_plan (launches 1 or 3; the parts' launch and the
 * normalising launch share the geometry). */
int t4k_softmax_axes_geometry(const int dim[4], int mask, int aligned, long ws_bytes, int out[8]);
/* k_nan_inf :278 / Tensor::has_nan tensor.cu:326-333: count of NaN/Inf -> *cnt_dev (int) */
int t4k_nan_inf(const float *src, long n, int *cnt_dev, t4k_stream_t s);
/* k_copy :134 */
int t4k_copy(const float *src, float *dst, long n, t4k_stream_t s);
/* k_transpose :150 (one sample): dst[(H*j+i)*C+c] = src[(W*i+j)*C+c]; bit-exact */
int t4k_transpose(const float *src, float *dst, int H, int W, int C, t4k_stream_t s);
/* k_identity :160 (one sample) */
int t4k_identity(float *dst, int H, int W, int C, t4k_stream_t s);
/* k_math :173 in-place unary / scalar op (LN/LOG clamp 1e-12, SQRT clamp 0, GFILL = v*j/n).  The clamps are fmaxf / fminf, which return
 * their other operand for a NaN: LN / LOG of NaN give the clamp's log (ln 1e-12, log10 1e-12); SQRT, RELU and SAT of NaN give 0. */
int t4k_math(int op, float *A, float v, long n, t4k_stream_t s);
/* k_ts_op :206  O = A op v,  op in {ADD,SUB,MUL,DIV} */
int t4k_ts_op(int op, const float *A, float v, float *O, long n, t4k_stream_t s);
/* k_tt_op :222  O = A op B */
int t4k_tt_op(int op, const float *A, const float *B, float *O, long n, t4k_stream_t s);
/* same with a second destination O2 (may be NULL): `out -= target` plus the pass-through copy `in = out` of a
 * final softmax/sigmoid layer (backprop.cu:129-131) in one launch */
int t4k_tt_op2(int op, const float *A, const float *B, float *O, float *O2, long n, t4k_stream_t s);
/* k_bce :248  *out_dev = sum t*ln(o+eps) + (1-t)*ln(1-o+eps), eps = 1e-6 */
int t4k_bce(const float *T, const float *O, long n, float *out_dev, t4k_stream_t s);
/* k_dot :309  O[c] = alpha*sum_k A[k*C+c]*B[k*C+c] + beta*O[c]  for c in [0,C) */
int t4k_dot(const float *A, const float *B, float *O, float alpha, float beta,
            int K, int C, t4k_stream_t s);
/* k_gemm_tile_claude :478 (Tensor::gemm3 tensor.cu:161, Tensor::linear :79):
 *   O[M,N,C] = alpha * op(A) @ op(B) + beta * O, per channel c (element stride C)
 *   op(A) = tA ? A stored [K,M,C] : A stored [M,K,C];  op(B) = tB ? B[N,K,C] : B[K,N,C]
 * fp32 accumulate on MFMA.  beta*O is read even when beta==0 (reference quirk, SURVEY a-1)
 * only if T4K_GEMM_BETA0_READS (default off: beta==0 never reads O). */
int t4k_gemm(const float *A, const float *B, float *O, float alpha, float beta,
             int tA, int tB, int M, int N, int K, int C, t4k_stream_t s);
/* k_gemm :370 / k_gemm_claude :411 (words gemm1/gemm2): double accumulator, tA/tB ignored */
int t4k_gemm_f64acc(const float *A, const float *B, float *O, float alpha, float beta,
                    int M, int N, int K, int C, t4k_stream_t s);
/* NumPy `@` over a batch (tenvm.cpp:277-287; _tdot :328-366 and Tensor::mm tensor.cu:161-180 loop one product per sample):
 *   O[b] = alpha * op(A[b]) @ op(B[b]) + beta * O[b]  for b in [0, batch), each a per-channel product with element stride C
 *   exactly as t4k_gemm.  A[b] = A + b*sA (sA == 0 broadcasts A over the batch), likewise B[b], O[b] (sO >= M*N*C when batch > 1).
 *   cA / cB: 1 when that operand has one channel serving all C output channels (stored without a channel axis), else C.
 * One launch per call, no allocation, no synchronisation (legal under capture); beta == 0 never reads O.  fp32 MFMA. */
int t4k_gemm_batched(const float *A, const float *B, float *O, float alpha, float beta, int tA, int tB,
                     int M, int N, int K, int C, int cA, int cB, int batch, long sA, long sB, long sO, t4k_stream_t s);
/* NumPy broadcasting for the arithmetic words (tenvm.cpp:277-287 names NumPy as the meaning of the tensor operators); no reference
 * definition: k_tt_op :222 takes two flat tensors of one size and Tensor::ten_op tensor.cu:28-53 loops one launch per sample.
 *   O[n,h,w,c] = A[n*sA[0] + h*sA[1] + w*sA[2] + c*sA[3]]  op  B[n*sB[0] + h*sB[1] + w*sB[2] + c*sB[3]],  op in {ADD,SUB,MUL,DIV}
 *   O is dense NHWC of extents dim = {N,H,W,C}; strides are in elements, a stride of 0 broadcasts that axis (the stride of an axis of
 *   extent 1 is not looked at).  Every element goes through k_tt_op's own expression: bit-identical to t4k_tt_op on operands expanded
 *   to the full shape.  O may alias an operand all of whose strides are the dense ones; it must not overlap a broadcast operand.
 * Exactly one launch per call, no allocation, no synchronisation (legal under capture); an empty dim is T4K_OK without a launch.
 * NULL, a negative extent or a negative stride: T4K_ERR_ARG; an unknown op: T4K_ERR_UNSUPPORTED. */
int t4k_tt_op_bcast(int op, const float *A, const float *B, float *O,
                    const int dim[4], const long sA[4], const long sB[4], t4k_stream_t s);
/* k_transpose :150 over a batch; no reference definition for the batch (the reference's `transpose` takes one rank-2 matrix).
 *   dst[b] = transpose(src[b]) for b in [0, batch): each entry [H,W,C] -> [W,H,C] exactly as t4k_transpose, entries H*W*C apart.
 * Bit-exact, one launch per call; batch == 0 is T4K_OK without a launch; H, W, C <= 0, batch < 0 or NULL: T4K_ERR_ARG. */
int t4k_transpose_batched(const float *src, float *dst, int H, int W, int C, int batch, t4k_stream_t s);
/* Any order of the four axes; no reference definition: the nearest thing is k_transpose :150, which swaps H and W of one sample.
 *   src is dense NHWC of extents dim = {N,H,W,C}; perm[i] is the source axis (0 = N ... 3 = C) that output axis i takes - NumPy's
 *   transpose(perm); dst is dense with extents dim[perm[i]].  Bit-exact: an element is loaded and stored and nothing else (NaN payloads
 *   and denormals survive).
 * Exactly one launch per call, whatever the order and the shape; no allocation, no synchronisation, no workspace (legal under capture).
 * NULL src / dst / dim / perm, an extent < 1, more than 2^40 elements, a perm that is not a permutation of 0..3, dst overlapping src
 * (dst == src included), or an extent above 2^32 left by the merge of neighbouring axes other than the contiguous run itself:
 * T4K_ERR_ARG. */
int t4k_permute(const float *src, float *dst, const int dim[4], const int perm[4], t4k_stream_t s);
/* The plan t4k_permute takes for (dim, perm) when both pointers are (aligned != 0) or are not 16-byte aligned; launches nothing and
 * needs no device.
 * out = { family (0 copy: nothing moves after the merge, 1 runs: the innermost group stays innermost, 2 tiles: a transpose through LDS),
 *         float4 path (0 / 1; always 0 for tiles),
 *         tiles: tile extent along the source's innermost group; copy / runs: lanes that share a run (256 = a chunk of a long run),
 *         tiles: tile extent along the output's innermost group; copy / runs: runs per 256-lane pass,
 *         work items (workgroup iterations; the grid is their count capped at 2048, the kernel strides over the rest),
 *         groups left after dropping extents of 1 and merging,
 *         tiles: entries of the inner batch group a tile takes (1 unless both tile sides are narrow); copy / runs: 1 }. */
int t4k_permute_plan(const int dim[4], const int perm[4], int aligned, int out[7]);
/* A box of one tensor onto a box of another; no reference definition: the nearest thing is MMU::slice mmu.cu:307-330, one memcpy per
 * (sample, row) of an H / W window.
 *   src is dense NHWC of extents sdim, dst dense NHWC of extents ddim; dst[doff + i] = src[soff + i] for every i with 0 <= i < ext on
 *   each axis, and no other element of dst is written.  A slice is doff = 0, ddim = ext; a store is soff = 0, sdim = ext; box to box
 *   is allowed.  Bit-exact: an element is loaded and stored and nothing else (NaN payloads and denormals survive).
 * Exactly one launch per call, whatever the box and the shapes; no allocation, no synchronisation, no workspace (legal under capture).
 * NULL src / dst / sdim / soff / ddim / doff / ext, an extent < 1, a negative offset, off + ext > dim on either side, more than 2^40
 * elements in either tensor, any overlap of the two tensors' whole byte ranges (dst == src included), or a digit of the run index
 * other than the outermost that the merge of neighbouring axes leaves at 2^32 or above: T4K_ERR_ARG. */
int t4k_window(const float *src, const int sdim[4], const int soff[4],
               float *dst, const int ddim[4], const int doff[4], const int ext[4], t4k_stream_t s);
/* The plan t4k_window takes for the two boxes when both base pointers are (aligned != 0) or are not 16-byte aligned; launches nothing and
 * needs no device (t4k_window itself looks at the two box starts, so base pointers that are off 16 bytes by what the offsets make up for
 * still take the float4 path).  Axes of extent 1 fold into the two box starts; an axis merges with its inner neighbour when that one is taken whole
 * on both sides (ext == sdim == ddim); what is left is R runs of L contiguous floats with at most three digits above them.
 * out = { family (0 copy: nothing is left above the run, 1 runs),
 *         float4 path (0 / 1: L % 4 == 0, every stride left a multiple of 4 and both box starts on 16 bytes),
 *         run length L in floats (saturated at 2^31 - 1),
 *         runs R (saturated likewise),
 *         digits of the run index (0..3),
 *         work items (256-lane passes, saturated likewise; the grid is their count capped at 2048, the kernel strides over the rest) }. */
int t4k_window_plan(const int sdim[4], const int soff[4], const int ddim[4], const int doff[4],
                    const int ext[4], int aligned, int out[6]);

/* ------------------------------------------------ linear algebra (t4math.cu) */
/* Tensor::inverse tensor.cu:344-369 (k_find_pivot/k_swap_rows/k_diag/k_elim :742-836):
 * Gauss-Jordan with partial pivoting on A[K,K] and I[K,K] in place; whole host loop runs
 * on the device.  *status_dev (int): 0 ok, z+1 = singular at column z. */
int t4k_inverse(float *A, float *I, int K, int *status_dev, t4k_stream_t s);
/* Tensor::plu tensor.cu:371-398 (k_lu_col :854, k_pivot :887): A -> packed L\U in place,
 * piv_dev[K] pivot rows; if I != NULL and I != A, apply the row swaps to I (=> P). */
int t4k_plu(float *A, float *I, int *piv_dev, int K, int *status_dev, t4k_stream_t s);
/* Tensor::lu_inverse tensor.cu:400-417 (k_fsub :904, k_bsub :920) */
int t4k_lu_inverse(float *A, float *I, int *piv_dev, int K, int *status_dev, t4k_stream_t s);
/* Tensor::lu tensor.cu:419-429 (k_lu :936): keep U (get_u) or unit-L of a packed L\U */
int t4k_lu_extract(float *LU, int get_u, int K, t4k_stream_t s);
/* k_logdet :952: *logdet_dev = sum ln|U[j,j]|, *sign_dev = prod sign(U[j,j]) */
int t4k_logdet(const float *LU, int K, float *logdet_dev, int *sign_dev, t4k_stream_t s);
/* The same over a BATCH of `batch` row-major K x K matrices, entry b at A + b*K*K (likewise X, Pm; piv_dev + b*K; status_dev[b]; det_dev[b]).
 * No reference definition for the batch: the reference's words take one rank-2 matrix (tenvm.cpp:134-216).  Exactly ONE kernel launch
 * per call whatever `batch` is, no allocation, no synchronisation; batch == 0 is T4K_OK and launches nothing.  Pivot rule and status as
 * the per-matrix entries: largest |a|, lowest row on a tie, |pivot| < 1e-6 = singular -> status_dev[b] = z + 1 (else 0).  A singular
 * entry does not stop the others; what it leaves in its outputs is unspecified, except det_dev[b] = 0.
 * Unlike the per-matrix entries, X and Pm are pure OUTPUTS: the kernel writes the identity itself.
 * K <= 0, batch < 0 or a NULL pointer: T4K_ERR_ARG; K > 1024: T4K_ERR_UNSUPPORTED. */
/* Tensor::inverse tensor.cu:344-369 (k_find_pivot/k_swap_rows/k_diag/k_elim :742-836); no reference definition for the batch.
 * X[b] = inverse(A[b]) by Gauss-Jordan.  A is scratch: K <= 140 leaves it untouched, above that it holds the eliminated rows (column z
 * of it is not maintained) - treat it as undefined after the call. */
int t4k_inverse_batched(float *A, float *X, int K, int batch, int *status_dev, t4k_stream_t s);
/* Tensor::plu tensor.cu:371-398 (k_lu_col :854, k_pivot :887); no reference definition for the batch.
 * A[b] -> packed L\U, piv_dev[b*K + z] = pivot row of column z (-1 at the singular column), Pm (may be NULL) = the permutation matrix P. */
int t4k_plu_batched(float *A, float *Pm, int *piv_dev, int K, int batch, int *status_dev, t4k_stream_t s);
/* Tensor::lu_inverse tensor.cu:400-417 (k_fsub :904, k_bsub :920); no reference definition for the batch.
 * A[b] -> packed L\U, X[b] = inverse(A[b]) by substitution on the columns of P. */
int t4k_lu_inverse_batched(float *A, float *X, int *piv_dev, int K, int batch, int *status_dev, t4k_stream_t s);
/* Tensor::lu tensor.cu:419-429 (k_lu :936); no reference definition for the batch. */
int t4k_lu_extract_batched(float *LU, int get_u, int K, int batch, t4k_stream_t s);
/* Tensor::det tensor.cu:431-456 (k_logdet :952); no reference definition for the batch.  A[b] -> packed L\U,
 * det_dev[b] = expf(sum ln|u_jj|) * (parity of the swaps) * (product of the signs of u_jj), finished on the device. */
int t4k_det_batched(float *A, int *piv_dev, int K, int batch, float *det_dev, int *status_dev, t4k_stream_t s);

/* ------------------------------------------------------- RNG (util.cu:28-70) */
/* Counter-based Philox4x32-10 replaces the reference's 1024 cuRAND XORWOW states
 * (distribution parity only; the reference seeds from time(), sys.cpp:37). */
/* The host keeps the stream position (seed, counter): an eager draw gets its slice as kernel arguments.  Draws recorded
 * between t4k_graph_begin/end read a device copy instead and advance it themselves, so every replay gets a fresh slice;
 * t4k_graph_launch keeps host and device positions in step.  t4k_rand_offset()/set_offset() are host-only and cheap. */
int t4k_rand_init(uint64_t seed);
/* d[i] = scale * (bias + u_i), u uniform (0,1] or N(0,1) (util.cu:58-70) */
int t4k_rand(float *d, long n, int opt, float bias, float scale, t4k_stream_t s);
/* The stream position is kept in whole Philox counters of 4 elements.  t4k_rand_set_offset(off) rounds `off` (in elements) DOWN to a
 * multiple of 4 - the remainder is dropped, not remembered - and t4k_rand_offset() always returns a multiple of 4: the position set, plus
 * 4 * ceil(n / 4) for every draw of n elements since (times `world` for a sample-keyed draw of a shard, below).  Offsets are 64-bit and
 * wrap mod 2^64; the counter's high word and the seed's high word are both part of the stream (element 2^34 is counter 2^32). */
uint64_t t4k_rand_offset(void);                    /* current stream offset (for checkpoint/tests) */
int t4k_rand_set_offset(uint64_t off);
uint64_t t4k_rand_seed(void);                      /* the seed of the stream (a host that embeds several VMs saves / restores (seed, offset) per VM) */
/* Data-parallel shard of the stream (SURVEY 8e "dropout: per-rank Philox offset = global sample index").  With a shard (rank, world)
 * set, a dropout-mask draw of n elements takes elements [rank*n, (rank+1)*n) of the n*world-element draw the whole batch would make
 * and moves the stream by n*world, so `world` ranks x batch B draw exactly the masks of one rank x batch B*world (n % 4 == 0; every
 * rank must make the same draws in the same order).  Every other draw (weight init, `rand` words) stays replicated.  t4k_comm_init
 * sets the shard to the communicator's (rank, world), t4k_comm_destroy resets it to (0, 1). */
int t4k_rand_set_shard(int rank, int world);
int t4k_rand_shard_world(void);                    /* 1 = no shard.  Sharded draws are keyed on the host per launch: a host must not replay captured graphs while world > 1 */
/* the mask of a dropout layer (Model::_fstep L_DROPOUT forward.cu:100-103 + t4_rand): uniform (0,1], keyed by sample as above */
int t4k_dropout_mask(float *mask, long n, t4k_stream_t s);

/* --------------------------------------------------- nn kernels (nn/nmath.*) */
/* k_bias nmath.cu:27  O[n,e] += B[e] */
int t4k_bias(const float *B, float *O, int N, int E0, t4k_stream_t s);
/* k_activate nmath.cu:37: layer in {RELU,TANH,SIGMOID,SELU,LEAKYRL,ELU,DROPOUT};
 * writes output O and derivative mask F (for DROPOUT, F holds uniform randoms on entry) */
int t4k_activate(int layer, const float *I, float *O, float *F, float alpha, long n, t4k_stream_t s);
/* k_softmax_small / k_softmax nmath.cu:74-169: row softmax over C per sample */
int t4k_softmax(const float *I, float *O, int N, int C, t4k_stream_t s);
/* Model::_flogsoftmax forward.cu:245-259 as written there: O[n,c] = exp(I[n,c]) - log10(max(sum_c exp(I[n,c]), 1e-6)) */
int t4k_logsoftmax(const float *I, float *O, int N, int C, t4k_stream_t s);
/* k_batchnorm_1/2/3 nmath.cu:177-264 (Model::_fbatchnorm forward.cu:263-309).
 * stat_dev[3C]: [0,C) rvar = 1/(sqrt(max(var,0))+1e-6), [C,2C) mean, [2C,3C) scratch */
int t4k_batchnorm_fwd(const float *I, float *O, float *XH, const float *W, const float *B,
                      float *stat_dev, int N, int HW, int C, t4k_stream_t s);
/* k_dbatchnorm_1/2/3 nmath.cu:295-414 (Model::_bbatchnorm backprop.cu:311-370):
 * dX = gamma*rvar*(dY - mean(dY) - xhat*mean(dY*xhat)); dB,dW += the MEANS (quirk a-17) */
int t4k_batchnorm_bwd(const float *W, const float *DY, const float *XH, float *DX,
                      float *DW, float *DB, float *stat_dev, int N, int HW, int C,
                      int train, t4k_stream_t s);
/* k_dlinear_db nmath.cu:274  DB[e] += sum_n DY[n,e] */
int t4k_dlinear_db(const float *DY, float *DB, int N, int E0, t4k_stream_t s);
/* k_conv2d<TS,KS,S,P> nmath.tcu:34 (Model::_fconv forward.cu:125-155):
 * O[n,i,j,c0] = B[c0] + sum F[((c1*K+ky)*K+kx)*C0+c0] * I[n,i*S+ky-P,j*S+kx-P,c1]
 * supported (K,S,P): (1,1,0) (3,1,1) (4,2,1) (5,1,2); output is written, not accumulated */
int t4k_conv2d_fwd(const float *I, float *O, const float *F, const float *B,
                   int N, int H1, int W1, int C1, int H0, int W0, int C0,
                   int K, int S, int P, t4k_stream_t s);
/* same, plus the copy of the batch the model's layer 0 keeps (`n0 = input`, forward.cu:39): ICOPY (may be NULL) receives
 * I, from the same launch when the layer takes the few-input-channel direct kernel */
int t4k_conv2d_fwd2(const float *I, float *ICOPY, float *O, const float *F, const float *B,
                    int N, int H1, int W1, int C1, int H0, int W0, int C0,
                    int K, int S, int P, t4k_stream_t s);
/* Model::_fconv followed by Model::_fbatchnorm (forward.cu:129-155, 263-309) - a conv layer with a batch-norm layer right behind it: Y = conv(I) (+ ICOPY as above),
 * then O / XH / stat_dev exactly as t4k_batchnorm_fwd(Y, ...) writes them.  One call so that the per-channel sums of Y can leave the conv kernel's epilogue
 * (where the layer's kernel carries them) instead of costing a separate pass over Y; otherwise it IS the two calls */
int t4k_conv2d_bn_fwd(const float *I, float *ICOPY, float *Y, const float *F, const float *Bc,
                      int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P,
                      float *O, float *XH, const float *W, const float *B, float *stat_dev, t4k_stream_t s);
/* k_dconv2d<TS,KS,S,P> nmath.tcu:211 (Model::_bconv backprop.cu:152-191):
 * DB[c0] += sum dO; DF += sum I*dO (both only if train);
 * DX (overwritten) scatter (i*S+ky-P, j*S+kx-P) += F[c1,K-1-ky,K-1-kx,c0]*dO  (flipped, quirk a-11).
 * DX == NULL computes dF|dB only, DF == DB == NULL computes dX only (lets the host fork them). */
int t4k_conv2d_bwd(const float *I, const float *DO, float *DX, const float *F,
                   float *DF, float *DB,
                   int N, int H1, int W1, int C1, int H0, int W0, int C0,
                   int K, int S, int P, int train, t4k_stream_t s);
/* same, with an optional second destination for dX: the reference keeps dX in the layer's scratch tensor and
 * then copies it over the layer input (`in = dx`, backprop.cu:185); DX2 receives that copy from the same launch */
int t4k_conv2d_bwd2(const float *I, const float *DO, float *DX, float *DX2, const float *F,
                    float *DF, float *DB,
                    int N, int H1, int W1, int C1, int H0, int W0, int C0,
                    int K, int S, int P, int train, t4k_stream_t s);
/* conv2d with RUN-TIME geometry (csrc/conv_geo.hip): what the reference leaves open - "TODO: stride, dilation" nmath.tcu:12, nmath.cu:269, nmath.h:25;
 * "TODO: dilation" model.cpp:125 - finished for k_conv2d / k_dconv2d nmath.tcu:12,34-104,211-338 and Model::_iconv model.cpp:124-137.
 * Admitted: K 1..7, S 1..4, D 1..4, 0 <= P <= D(K-1), H0 == (H1 + 2P - D(K-1) - 1)/S + 1 >= 1 (W likewise), every extent >= 1, N H0 W0 and N H1 W1
 * below 2^31, one dF | dB slab ((C1 K K + 1) C0 floats) within half the stream workspace.  An extent below 1, a NULL tensor or an H0 / W0 that the
 * geometry does not give: T4K_ERR_ARG; a geometry outside the set: T4K_ERR_UNSUPPORTED; either leaves a t4k_last_error text and writes nothing.
 * The four geometries of t4k_conv2d_fwd (D = 1) are admitted too and run on THESE kernels, not the specialised ones.
 *   O[n,i,j,c0] = B[c0] + sum F[((c1*K+ky)*K+kx)*C0+c0] * I[n,i*S+ky*D-P,j*S+kx*D-P,c1]     (zero border; O is written once, not accumulated)
 * ICOPY (may be NULL) receives I as in t4k_conv2d_fwd2, by a copy command.  One kernel launch; no allocation, no synchronisation (legal under capture). */
int t4k_conv2d_geo_fwd(const float *I, float *ICOPY, float *O, const float *F, const float *B,
                       int N, int H1, int W1, int C1, int H0, int W0, int C0,
                       int K, int S, int P, int D, t4k_stream_t s);
/* its backward (k_dconv2d nmath.tcu:211-338 finished for nmath.tcu:12): DB[c0] += sum dO, DF += sum I*dO (both only if train); DX (overwritten, every
 * element stored exactly once) and the optional second copy DX2, which may be I itself (`in = dx`, backprop.cu:185: dF | dB read I first).
 * DX == NULL: dF | dB only; DF == DB == NULL: dX only - as t4k_conv2d_bwd2.
 * DX is the TEXTBOOK gradient, dX[n,y,x,c1] = sum F[c1,ky,kx,c0] * dO[n,i,j,c0] over the taps with i*S + ky*D - P == y, j*S + kx*D - P == x - what
 * autograd gives - NOT the rotated-filter dX of t4k_conv2d_bwd (quirk a-11), which stays with the four geometries the reference itself computes:
 * for geometries it never computes there is nothing to be faithful to.  On those four, this DX equals t4k_conv2d_bwd's DX of the filter rotated by 180 degrees.
 * At most three launches (slabs, their fold, dX), one for dX alone; fixed summation order, no atomics. */
int t4k_conv2d_geo_bwd(const float *I, const float *DO, float *DX, float *DX2, const float *F,
                       float *DF, float *DB,
                       int N, int H1, int W1, int C1, int H0, int W0, int C0,
                       int K, int S, int P, int D, int train, t4k_stream_t s);
/* The plan the two entries above take (nmath.tcu:12,34-104,211-338; model.cpp:124-137) when the tensors the 16-byte paths read - I and F of the forward; dO, F and I of the backward - are ALL on 16 bytes (aligned bit 0 set) or are not,
 * and DB lies right behind DF (DB == DF + C1 K K C0: a layer's gradient block; aligned bit 1 clear) or does not (bit 1 set);
 * pure host arithmetic: launches nothing, needs no device; the launch code calls the same function.  Admission and return codes as above.
 * out = { forward channel tile (64 | 128; the pixel tile is 128),
 *         forward load path (bit 0: 16-byte gather of I - C1 % 4 == 0 and aligned; bit 1: 16-byte loads of F - C0 % 4 == 0 and aligned),
 *         dX channel tile (64 | 128), dX load path (1: 16-byte loads of dO and F - C0 % 4 == 0 and aligned),
 *         dF load path (bit 0: 16-byte loads of dO; bit 1: a tile's rows are the channels of ONE tap and I is gathered 16 bytes at a time -
 *                       C1 % 4 == 0, C1 >= 32, bit 0; otherwise the rows are (c1, ky, kx) side by side and I is gathered by dwords),
 *         dF slices (pixel slices of whole 32-pixel stages aiming at 1024 workgroups over the 64 x 64 tiles, shrunk until the slabs fit 8 MiB of workspace -
 *                    down to one, which may take the 32 MiB),
 *         the fold behind them (1: k_fold_add - up to 32 slices and DB right behind DF, because it walks whole slabs into one destination; 2: k_conv_df_fold),
 *         launches of a whole backward (3) }. */
int t4k_conv2d_geo_plan(int N, int H1, int W1, int C1, int C0, int K, int S, int P, int D,
                        int aligned, int out[8]);
/* Grouped and depthwise conv2d with RUN-TIME geometry (csrc/conv_group.hip): the entries above with the channels cut into G groups.  The reference has
 * NO groups - Model::_iconv model.cpp:121-180 allocates the dense T4(C1, K, K, C0) and k_conv2d ("TODO: stride, dilation" nmath.tcu:12) walks every input
 * channel - so there is no quirk to keep: this finishes those two for torch's conv2d(groups=G).  With Cg1 = C1 / G and Cg0 = C0 / G, output channel c0
 * belongs to group g = c0 / Cg0, F = T4(Cg1, K, K, C0):
 *   O[n,i,j,c0] = B[c0] + sum_{cg < Cg1, ky, kx} F[((cg*K+ky)*K+kx)*C0+c0] * I[n,i*S+ky*D-P,j*S+kx*D-P,g*Cg1+cg]     (zero border; O is written once, not accumulated)
 * = torch.nn.functional.conv2d(groups=G) with weight[c0][cg][ky][kx] = F[cg,ky,kx,c0].
 * Admitted: the geometries of t4k_conv2d_geo_fwd (K 1..7, S 1..4, D 1..4, 0 <= P <= D(K-1), H0 == (H1 + 2P - D(K-1) - 1)/S + 1 >= 1, W likewise, N H0 W0 and
 * N H1 W1 below 2^31), 1 <= G with C1 % G == 0 and C0 % G == 0, one dF | dB slab ((Cg1 K K + 1) C0 floats) within 32 MiB, Cg1 and the channel tiles of the dF grid (C0 / 128, dwords: C0 / 32) within 65535 - anything else:
 * T4K_ERR_UNSUPPORTED.
 * An extent below 1, a NULL tensor or an H0 / W0 that the geometry does not give: T4K_ERR_ARG.  Either leaves a t4k_last_error text and writes nothing.
 * G == 1 is admitted and runs on THESE kernels (the host never sends it: a dense layer stays with the entries above).
 * ICOPY (may be NULL) receives I by a copy command.  One kernel launch; no allocation, no synchronisation (legal under capture). */
int t4k_conv2d_grp_fwd(const float *I, float *ICOPY, float *O, const float *F, const float *B,
                       int N, int H1, int W1, int C1, int H0, int W0, int C0,
                       int K, int S, int P, int D, int G, t4k_stream_t s);
/* its backward (k_dconv2d nmath.tcu:211-338 finished likewise; the reference has no groups): the TEXTBOOK gradients, what autograd gives.
 * DB[c0] += sum dO, DF[cg,ky,kx,c0] += sum I[.., g*Cg1+cg] * dO[.., c0] (both only if train); DX (overwritten, every element stored exactly once - an
 * input pixel no window covers gets 0) sums, for input channel c1 of group g, the Cg0 output channels of that group in ascending order; the optional
 * second copy DX2 may be I itself (dF | dB read I first).  DX == NULL: dF | dB only; DF == DB == NULL: dX only; DF and DB go together.
 * At most three launches (slabs, their fold, dX), one for dX alone; fixed summation order, no atomics; the slabs live in the stream workspace half that
 * t4k_conv2d_geo_bwd uses and are folded by the same two kernels. */
int t4k_conv2d_grp_bwd(const float *I, const float *DO, float *DX, float *DX2, const float *F,
                       float *DF, float *DB,
                       int N, int H1, int W1, int C1, int H0, int W0, int C0,
                       int K, int S, int P, int D, int G, int train, t4k_stream_t s);
/* The plan the two entries above take (the reference has no groups: model.cpp:121-180, nmath.tcu:12) when EVERY tensor a 16-byte path touches - I, F and O
 * of the forward; dO, F, I, DX and DX2 of the backward - is on 16 bytes (aligned bit 0 set) or is not, and DB lies right behind DF (DB == DF + Cg1 K K C0;
 * aligned bit 1 clear) or does not (bit 1 set); pure host arithmetic: launches nothing, needs no device; the launch code calls the same function.
 * Admission and return codes as above; a refusal writes nothing into out.
 * out = { engine (1: depthwise, Cg1 == 1; 2: general, an inner loop over the Cg1 input channels of the group),
 *         load path of the forward and of the dF | dB kernel: 0 one channel per thread, dwords; the others need C0 % 4 == 0 and bit 0 and give a thread 4
 *                   consecutive output channels, 16-byte loads of F and dO and 16-byte stores - 1: depthwise with multiplier 1, the four inputs are ONE
 *                   16-byte load of I per tap; 2: Cg0 % 4 == 0, the four channels lie in one group and share one dword of I per (cg, tap); 3: depthwise
 *                   with another multiplier, four dwords of I per tap,
 *         channels of a dX thread (4: load path 1, 16-byte loads of dO and F; 1 otherwise),
 *         channel lanes of a dF workgroup (a power of two up to 32; its other 256 / lanes rows are K tap rows x pixel sub-slices),
 *         pixel sub-slices of a dF workgroup ((256 / lanes) / K, added through LDS in ascending order),
 *         dF slices (pixel slices of whole 32-pixel stages aiming at 1024 workgroups over Cg1 x channel tiles, shrunk until the slabs fit 8 MiB of
 *                    workspace - down to one, which may take the 32 MiB),
 *         the fold behind them (1: k_fold_add - up to 32 slices and DB right behind DF; 2: k_conv_df_fold),
 *         launches of a whole backward (3) }. */
int t4k_conv2d_grp_plan(int N, int H1, int W1, int C1, int C0, int K, int S, int P, int D, int G,
                        int aligned, int out[8]);
/* Transposed convolution layer (word `dconv2d`, L_DCONV; allocation Model::_iconv txn model.cpp:121-180, dispatch forward.cu:110 /
 * backprop.cu:137 - the reference routes the layer's forward through the conv backward routine and vice versa but never finished it, see
 * csrc/dconv.hip).  I[N,H1,W1,C1] -> O[N,H0,W0,C0], F = T4(C1,K,K,C0), (H0-K+2P)/S+1 == H1:
 *   O[n,i*S+ky-P,j*S+kx-P,co] = B[co] + sum_ci F[ci,ky,kx,co] * I[n,i,j,ci]        (= torch ConvTranspose2d, weight[ci][co][ky][kx]) */
int t4k_dconv2d_fwd(const float *I, float *O, const float *F, const float *B,
                    int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P, t4k_stream_t s);
/* its backward: DX (overwritten) = conv(DO, F) with the same taps, DF += I x DO, DB[co] += sum DO (DF, DB only if train);
 * DX == NULL or DF == DB == NULL as for t4k_conv2d_bwd */
int t4k_dconv2d_bwd(const float *I, const float *DO, float *DX, const float *F, float *DF, float *DB,
                    int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P, int train, t4k_stream_t s);
/* k_pool<KS> nmath.tcu:122 (layer in AVGPOOL/MAXPOOL/MINPOOL/USAMPLE), KS in {2,3} */
int t4k_pool(int layer, const float *I, float *O, int N, int H1, int W1, int H0, int W0, int C,
             int KS, t4k_stream_t s);
/* k_dpool<KS> nmath.tcu:475: in place on the forward-input buffer I (reads x, zeroes the
 * tile, writes dy at the first arg-max/min; avg: dy/KS^2; usample: broadcast) */
int t4k_dpool(int layer, float *I, const float *DY, int N, int H1, int W1, int H0, int W0, int C,
              int KS, t4k_stream_t s);
/* avg / max / min pooling with RUN-TIME geometry (csrc/pool_geo.hip): what k_pool / k_dpool nmath.tcu:400-568 and Model::_ipool model.cpp:261 leave
 * out - their window is the stride, 2 or 3, without padding.  Admitted: layer AVGPOOL / MAXPOOL / MINPOOL, K 1..16, S 1..16, 0 <= P <= K/2, K <= H1 + 2P and
 * K <= W1 + 2P, N H1 W1 and N H0 W0 below 2^31 - otherwise T4K_ERR_UNSUPPORTED; an extent below 1: T4K_ERR_ARG.  A FLOOR grid, H0 == (H1 + 2P - K)/S + 1 and
 * W0 == (W1 + 2P - K)/S + 1 (from W1).  Pure host arithmetic: launches nothing, needs no device; the launch code calls the same function.
 * out = { H0, W0, channel vector width of the forward (4 | 1), of the backward (4 | 1) };
 * aligned bit 0: I and O on 16 bytes (and CODE, where given, on 4), bit 1: DY and DX on 16 bytes (and CODE on 4); a width of 4 also needs C % 4 == 0 */
int t4k_pool_geo_plan(int layer, int N, int H1, int W1, int C, int K, int S, int P, int aligned, int out[4]);
/* the forward (k_pool nmath.tcu:400-474 finished for any window, stride and padding; Model::_ipool model.cpp:261).  Window (i, j) covers rows
 * i*S - P .. i*S - P + K - 1, columns likewise; every channel on its own.  max / min: the extreme of the cells INSIDE the image, the first one in
 * (ky, kx) row-major order by a strict compare (torch max_pool2d, ties included); avg: (sum of the cells inside the image) / (float)(K K) - padding counts
 * as zeros, torch's count_include_pad=True.  NaN operands: unspecified.
 * CODE (may be NULL: inference, avg) receives the winning tap ky*K + kx of every output element as one byte, [n][i][j][c] with a pixel pitch of
 * 4 ceil(C / 4) bytes, the pad bytes written as 0; avg stores none.  An H0 / W0 that the rule does not give, a NULL I or O: T4K_ERR_ARG.
 * One launch; no allocation, no synchronisation (legal under capture). */
int t4k_pool_geo_fwd(int layer, const float *I, float *O, unsigned char *CODE,
                     int N, int H1, int W1, int C, int H0, int W0, int K, int S, int P, t4k_stream_t s);
/* its backward (k_dpool nmath.tcu:475-568 finished likewise; model.cpp:261): the TEXTBOOK gradient, dX[n,y,x,c] = sum of DY[n,i,j,c] over the windows
 * whose winning tap is (y, x) (max / min, from CODE - required, else T4K_ERR_ARG) or (sum of DY over the covering windows) / (float)(K K) (avg; CODE
 * ignored), the windows in ascending (i, j) order, no atomics: the same bits on every run.  EVERY element of DX is stored exactly once - a cell that
 * no window covers (S > K, rows / columns behind the last window) gets 0, where t4k_dpool leaves the forward value.  The forward input is not read:
 * DX may be its buffer (the in-place convention of t4k_dpool without its race on overlapping windows); DY must not overlap DX.
 * One launch; no allocation, no synchronisation. */
int t4k_pool_geo_bwd(int layer, const unsigned char *CODE, const float *DY, float *DX,
                     int N, int H1, int W1, int C, int H0, int W0, int K, int S, int P, t4k_stream_t s);
/* up-sampling by any integer factor (csrc/upsample.hip): what _iup model.cpp:294-310 (2x2 and 3x3 only), `const int me = in.iparm; ///< upsample method, TODO`
 * forward.cu:318 / backprop.cu:289 and the enum of ntypes.h:53-58, which no kernel reads, leave out.  The methods are that enum's. */
enum { T4K_UP_NEAREST = 0, T4K_UP_LINEAR, T4K_UP_BILINEAR, T4K_UP_CUBIC };   /* ntypes.h:53-58 */
/* The rule, separable and the same on both axes: H0 == K H1, W0 == K W1 (from W1); output row i = q K + r, 0 <= r < K, reads T taps at input rows
 * clamp(q + base[r] + a, 0, H1 - 1), a = 0 .. T - 1, with weights wt[r][a]:
 *   nearest (T 1): base 0, {1}                                                                   torch interpolate(scale_factor=K, mode='nearest')
 *   linear = bilinear (T 2): u = 2r + 1 - K; u >= 0: base 0, l = u / 2K, else base -1, l = (u + 2K) / 2K; {1 - l, l}        mode='bilinear', align_corners=False
 *   cubic (T 4): that base - 1 and l; {c2(l + 1), c1(l), c1(1 - l), c2(2 - l)}, the cubic-convolution polynomials with A = -0.75  mode='bicubic', align_corners=False
 * Admitted: method 0..3, K 1..16 (cubic 1..8: the 64-float table), N H0 W0 below 2^31 - otherwise T4K_ERR_UNSUPPORTED; an extent below 1: T4K_ERR_ARG.
 * Pure host arithmetic: launches nothing, needs no device; the launch code calls the same function.
 * out = { H0, W0, channel vector width of the forward (4 | 1), of the backward (4 | 1) }; aligned bit 0: I and O on 16 bytes, bit 1: DY and DX on 16 bytes; a
 * width of 4 also needs C % 4 == 0.  wt[r * 4 + a] and base[r] (either may be NULL) receive the table the kernels take: l as a rational, the polynomials
 * in double, each weight rounded once to float; unused cells 0. */
int t4k_upsample_plan(int method, int N, int H1, int W1, int C, int K, int aligned, int out[4], float wt[64], int base[16]);
/* the forward (_fupsample forward.cu:318 finished for any factor and for the method it ignores): every channel on its own,
 * O[n,i,j,c] = sum_a sum_b (wt[ri][a] wt[rj][b]) I[n, row_a, col_b, c] in ascending (a, b) order.  NaN operands: unspecified.
 * An H0 / W0 that the rule does not give, a NULL I or O: T4K_ERR_ARG.  One launch; no allocation, no synchronisation (legal under capture). */
int t4k_upsample_fwd(int method, const float *I, float *O, int N, int H1, int W1, int C, int H0, int W0, int K, t4k_stream_t s);
/* its backward (_bupsample backprop.cu:285-300 finished likewise; where the 2x2 / 3x3 route takes t4k_pool(AVGPOOL) and a scale map, this is ONE launch): the transpose of the forward
 * map, clamped taps included - a border row of DX collects every tap that was clamped onto it -, summed in ascending (i, j) order without atomics: the
 * same bits on every run, every element of DX stored exactly once.  The forward input is not read: DX may be its buffer (the in-place convention of
 * t4k_pool_geo_bwd); DY must not overlap DX.  One launch; no allocation, no synchronisation. */
int t4k_upsample_bwd(int method, const float *DY, float *DX, int N, int H1, int W1, int C, int H0, int W0, int K, t4k_stream_t s);
/* group / layer / instance norm on NHWC fp32 (csrc/groupnorm.hip): torch.nn.functional.group_norm(x, G, W, B, eps) with 1 <= G <= C,
 * C % G == 0, Cg = C / G, E = HW Cg; the group of channel c is c / Cg.  G = 1 is layer norm over (H, W, C) with a per-channel affine, G = C instance norm.
 * The reference has no such layer.  mean and the BIASED variance are per (sample, group); the variance is a sum of squared deviations from the group's own
 * computed mean (Chan's merge of (count, mean, M2) where a group is cut into parts), never E[x^2] - mean^2; rstd = 1 / sqrt(var + eps), eps INSIDE the root.
 * Admission and the plan, on the host alone (no device needed; the entries call the same function).  An extent below 1, NULL out or ws_bytes < 0: T4K_ERR_ARG;
 * G < 1, C % G != 0, N HW C or N G at or above 2^31, or partial slabs that do not fit ws_bytes: T4K_ERR_UNSUPPORTED; out is untouched then.
 * out = { rung (1 wave, 2 workgroup, 3 stream, 4 split), load path (4 = 16 bytes per lane, 1 = dwords), groups per workgroup, parts per group,
 *         forward launches, dW | dB slices, fold kind (1 fold_add, 2 df_fold), backward launches with train != 0 };
 * aligned != 0: every pointer of the call on 16 bytes; the 16-byte path also needs Cg % 4 == 0 */
int t4k_groupnorm_plan(int N, int HW, int C, int G, int aligned, long ws_bytes, int out[8]);
/* the forward: XH = (I - mean) rstd, O = XH W[c] + B[c]; STAT (4 N G floats: mean | rstd | s1 | s2, each N G long) receives mean and rstd.
 * O and XH are written once per element; O may be I.  eps <= 0 or a NULL tensor: T4K_ERR_ARG.  One launch (two on the split rung); no atomics, the same bits
 * on every call; no allocation, no synchronisation.  A refusal leaves a t4k_last_error text and writes nothing. */
int t4k_groupnorm_fwd(const float *I, float *O, float *XH, const float *W, const float *B, float *STAT,
                      int N, int HW, int C, int G, float eps, t4k_stream_t s);
/* its backward, the textbook one: t = W[c] DY, s1 = mean_g t, s2 = mean_g (t XH), DX = rstd (t - s1 - XH s2); STAT's rstd is read, its s1 | s2 written.
 * train != 0: DW[c] += sum_{n,h,w} DY XH and DB[c] += sum DY (SUMS), through per-slice slab rows in the stream's workspace and a fold launch; train == 0
 * leaves both untouched and both may be NULL.  DX is written once per element and may be DY. */
int t4k_groupnorm_bwd(const float *W, const float *DY, const float *XH, float *STAT, float *DX,
                      float *DW, float *DB, int N, int HW, int C, int G, int train, t4k_stream_t s);
/* multi-head scaled-dot-product attention on NHWC fp32 tokens (csrc/attention.hip): torch's scaled_dot_product_attention(q, k, v, is_causal)
 * on qkv.reshape(B, L, 3, heads, d).  The reference has no such layer (its README lists "Transformer: developing" for v5.0).  QKV is [N, L, 3E], E = heads d, a
 * token's channels [ Q(E) | K(E) | V(E) ], head h owning channels h d .. (h + 1) d - 1 of each E; O is [N, L, E] in the same head order; LSE is [N, heads, L].
 * With scale = (float)(1 / sqrt((double)d)): S_ij = scale sum_k Q_ik K_jk (causal != 0: keys j <= i only), m_i = max_j S_ij, l_i = sum_j exp(S_ij - m_i),
 * Y_ic = sum_j exp(S_ij - m_i) V_jc / l_i, LSE_i = m_i + ln l_i.  No dropout, no other mask; exp is __expf.
 * Admission and the plan, on the host alone (no device needed; the entries call the same function).  An extent below 1, NULL out or ws_bytes < 0: T4K_ERR_ARG;
 * d outside 4 .. 128 or d % 4 != 0, N L 3E at or above 2^31, or 4 N heads L bytes of row sums that do not fit ws_bytes: T4K_ERR_UNSUPPORTED; out is untouched then.
 * out = { rung (1: d <= 16, 2: d <= 32, 3: d <= 64, 4: d <= 128 - the head size the kernels pad to), load path (4 = 16 bytes per lane, 1 = dwords),
 *         query tile BQ, key tile BK, forward launches, backward launches, workgroups of the forward, workspace bytes used };
 * aligned != 0: every pointer of the call on 16 bytes (d % 4 == 0 makes every row of every head so) */
int t4k_attention_plan(int N, int L, int heads, int d, int causal, int aligned, long ws_bytes, int out[8]);
/* the forward.  O and OK (where not NULL) receive the same values, each element written once: OK is the copy the backward reads once O's buffer holds dY.
 * LSE is written once per (n, head, token).  A workgroup owns (n, head, BQ queries); K and V stream through LDS in tiles of BK keys; both products on fp32 MFMA,
 * the online max / sum with the rescale of the running output; S and P never reach memory.  A causal call visits no key tile wholly above the diagonal.
 * One launch; no atomics, a fixed summation order, the same bits on every call; no allocation, no synchronisation.  A NULL QKV, O or LSE: T4K_ERR_ARG.
 * A refusal leaves a t4k_last_error text and writes nothing. */
int t4k_attention_fwd(const float *QKV, float *O, float *OK, float *LSE, int N, int L, int heads, int d, int causal, t4k_stream_t s);
/* its backward, the textbook one (torch autograd of the above): D_i = sum_c DY_ic OK_ic, P_ij = exp(S_ij - LSE_i) recomputed, dP_ij = sum_c DY_ic V_jc,
 * dS_ij = P_ij (dP_ij - D_i), dV_jc = sum_i P_ij DY_ic, dQ_ik = scale sum_j dS_ij K_jk, dK_jk = scale sum_i dS_ij Q_ik.  DQKV has QKV's layout and is written
 * once per element; it must not overlap QKV, OK or DY (an overlap of the stated extents: T4K_ERR_ARG).  Two launches: the pass that owns query tiles (D into the
 * stream's workspace, dQ) and the pass that owns key tiles (dK, dV); no atomics, the same bits on every call; no allocation, no synchronisation. */
int t4k_attention_bwd(const float *QKV, const float *OK, const float *DY, const float *LSE, float *DQKV,
                      int N, int L, int heads, int d, int causal, t4k_stream_t s);
/* add & norm on NHWC fp32 tokens (csrc/addnorm.hip): out = norm(x + skip), either half optional.  The reference has neither a residual
 * connection nor a per-token norm (its README lists "add block - residual map" as to do).  rows = N H W tokens of C contiguous floats; z = X + S (S NULL: z = X).
 * mode 0: O = z.  mode 1, torch's layer_norm(z, (C,), W, B, eps): mean = sum_c z / C, var = sum_c (z - mean)^2 / C (centred on the token's own computed
 * mean), rstd = 1 / sqrt(var + eps), xhat = (z - mean) rstd.  mode 2, RMS norm: rstd = 1 / sqrt(sum_c z^2 / C + eps), xhat = z rstd.  Both: O = xhat W[c] + B[c]
 * (a B left at 0 is plain RMS norm).
 * Admission and the plan, on the host alone (no device needed; the entries call the same function).  An extent below 1, a mode outside 0..2, NULL out or
 * ws_bytes < 0: T4K_ERR_ARG; rows or rows C at or above 2^31, a mode != 0 with C above 8192 (16-byte path) or 2048 (dwords), or a workspace that does not
 * hold one slab row of 2 C floats: T4K_ERR_UNSUPPORTED; out is untouched then.
 * out = { rung (0: mode 0, flat; 1: a team of T lanes of a wave per token; 2: a workgroup per token), load path (4 = 16 bytes per lane: aligned != 0 and
 *         C % 4 == 0; else 1 = dwords), tokens a workgroup holds at a time (0 on rung 0), lanes per token T (8, 16, 32, 64: the smallest that leaves a lane at
 *         most 8 items of the load width; 256 on rung 2; 0 on rung 0), forward launches (1), dW | dB slab rows (one per workgroup of the backward: at most 1024
 *         and at most what ws_bytes holds, whatever rows is; 0 on rung 0), fold kind (1: a thread per output walks the rows, 2: a wave per output; 0 on rung
 *         0), backward launches with train (2; 1 on rung 0) };  aligned != 0: every pointer of the call on 16 bytes */
int t4k_addnorm_plan(long rows, int C, int mode, int aligned, long ws_bytes, int out[8]);
/* the forward.  S may be NULL; with mode 0, XH, RSTD, W and B may be NULL (they are ignored).  O and XH ([rows, C]) are written once per element, RSTD ([rows])
 * once per token.  O may be X or S (the tensor itself: a thread stores only what it loaded, after all its loads of the token); any other overlap of an output
 * with another operand that the pointers and extents show, a NULL X or O, eps <= 0: T4K_ERR_ARG.  One launch; no atomics, a fixed summation order, the same
 * bits on every call; a token's results depend on that token alone, so any split of the rows gives the same bits.  No allocation, no synchronisation
 * (legal under capture).  A refusal leaves a t4k_last_error text and writes nothing. */
int t4k_addnorm_fwd(const float *X, const float *S, float *O, float *XH, float *RSTD, const float *W, const float *B,
                    long rows, int C, int mode, float eps, t4k_stream_t s);
/* its backward.  t = DY + DY2 (DY2: the gradient that arrives over a skip tapping this layer's output; NULL: none).  mode 0: DX = t.  Else g = W t,
 * mode 1: DX = rstd (g - mean_c(g) - xhat mean_c(g xhat)), mode 2: DX = rstd (g - xhat mean_c(g xhat)); DW[c] += sum_rows t xhat, DB[c] += sum_rows t (SUMS)
 * when train != 0 - otherwise, and with mode 0, DW and DB are untouched and may be NULL.  DX is written once per element and may be DY or DY2 (the tensor
 * itself); any other overlap: T4K_ERR_ARG.  A workgroup leaves one row of 2 C partial sums in the first half of the stream's workspace, a second launch
 * folds the rows in a fixed order: one launch, two with train.  The skip source of the forward receives the same DX: the caller hands it on as that
 * layer's DY2. */
int t4k_addnorm_bwd(const float *W, const float *DY, const float *DY2, const float *XH, const float *RSTD, float *DX,
                    float *DW, float *DB, long rows, int C, int mode, int train, t4k_stream_t s);
/* the embedding layer on NHWC fp32 tokens (csrc/embed.hip): a token-embedding lookup, a learned position table, or both.  The reference has
 * no such layer.  T = N L tokens of E contiguous floats, t = n L + l.  Token mode (V >= 1): IDS[T] holds the ids as floats; valid(t) <=> x_t >= 0 and x_t < V
 * in float compares (NaN, negatives, -0.5, V, 1e9, +-inf are not valid), id_t = (int)x_t, formed only where valid;  O[t, :] = (valid(t) ? TABLE[id_t, :] : 0)
 * + (POS ? POS[l, :] : 0).  An id that is not valid is padding: a zero token vector, no gradient, no access (torch's embedding(padding_idx)).  Position mode
 * (V = 0): O[t, :] = X[t, :] + POS[l, :].  TABLE is [V, E], POS [L, E].
 * Admission and the plan, on the host alone (no device needed; the entries call the same function), a function of its arguments only.  An extent below 1 (V
 * may be 0), T % L != 0, NULL out, ws_bytes < 0, pos outside 0..1, V = 0 with pos = 0: T4K_ERR_ARG; T E or V E at or above 2^31: T4K_ERR_UNSUPPORTED; out is
 * untouched then.
 * out = { rung (0: position mode; 1: token mode, P = 1, a unit adds onto DTABLE itself; 2: token mode, P > 1, partial rows and a fold), load path (4 = 16
 *         bytes per lane: aligned != 0 and E % 4 == 0; else 1 = dwords), table rows of a slab R (16; 0 in position mode), token parts P (1 unless the
 *         vocabulary alone gives fewer than 1024 wave units: then min(ceil(1024 / units), T / 64, min(ws_bytes, 2^31 - 1) / (4 V E)), at least 1, re-counted from whole
 *         64-id loads per part), forward launches (1), backward launches with train (the rung; 1 in position mode), workgroups of the scatter launch (four
 *         wave units each, a unit = R rows x 64 lanes of the load width x one part, plus ceil(L (E / width) / 16) for the dPOS role where pos != 0),
 *         workspace bytes used (4 P V E where P > 1, else 0) };  aligned != 0: every pointer of the call on 16 bytes */
int t4k_embed_plan(long T, int L, int V, int E, int pos, int aligned, long ws_bytes, int out[8]);
/* the forward.  Exactly one of IDS (token mode: V >= 1, TABLE required) and X (position mode: V = 0, POS required, TABLE NULL) is non-NULL; POS NULL: no
 * position term.  O [T, E] is written once per element and must not overlap another operand (T4K_ERR_ARG).  One launch; the id is read once per token; the
 * output is streamed.  At most one fp32 add per element: the same bits as the rule restated in float32.  No allocation, no synchronisation (legal under
 * capture).  A refusal leaves a t4k_last_error text, launches nothing and writes nothing. */
int t4k_embed_fwd(const float *IDS, const float *X, const float *TABLE, const float *POS, float *O,
                  long T, int L, int V, int E, t4k_stream_t s);
/* its backward.  DTABLE[v, :] += sum over the valid t with id_t = v of DY[t, :], DPOS[l, :] += sum over n of DY[n L + l, :] (SUMS) when train != 0 -
 * otherwise both are untouched and may be NULL; DPOS NULL with train: no position table.  Token mode (V >= 1, IDS required): no dX, DX is ignored and the
 * ids are left as they are.  Position mode (V = 0, IDS NULL, DX required): DX = DY, read by the same load as the sum; DX may be DY itself.  Any other overlap
 * of an output with another operand: T4K_ERR_ARG.  Ownership by table row: a wave unit walks its part of the ids in ascending token order and adds the dY
 * rows of its slab in that order; rung 2 leaves [P, V, E] partial rows in the first half of the stream's workspace and a second launch adds them in part
 * order.  A table element whose sum is exactly 0 is not written (a row no token names keeps its bits).  No atomics, the same bits on every call; no
 * allocation, no synchronisation.  train == 0: token mode launches nothing, position mode copies DY to DX unless they are one tensor. */
int t4k_embed_bwd(const float *IDS, const float *DY, float *DTABLE, float *DPOS, float *DX,
                  long T, int L, int V, int E, int train, t4k_stream_t s);
/* k_sgd nmath.cu:419: dg=DG/Nw; beta~0: G-=lr*dg else M=b*M+(1-b)*dg, G-=lr*M; DG=0 */
int t4k_sgd(float *G, float *DG, float *M, int Nw, float lr, float beta, long n, t4k_stream_t s);
/* k_adam nmath.cu:438 (no bias correction, eps outside sqrt): zeroes DG */
int t4k_adam(float *G, float *DG, float *M, float *V, float lr, float b1, float b2,
             long n, t4k_stream_t s);
/* k_adamw nmath.cu:456 */
int t4k_adamw(float *G, float *DG, float *M, float *V, float lr, float b1, float b2, float wd,
              long n, t4k_stream_t s);
/* Model::backprop's start for an output layer with a derivative mask (tanh / relu / ... as the last op: backprop.cu:43-53 copies
   the target into the output tensor, _bactivate :256-263 multiplies by the mask): OUT[i] = T[i], IN[i] = T[i] * MASK[i] */
int t4k_copy_mask(const float *T, const float *MASK, float *OUT, float *IN, long n, t4k_stream_t s);
/* Model::broadcast backprop.cu:17-29: O[N,E] with O[n,e] = T[n] (a per-sample target spread over the output width) */
int t4k_broadcast_rows(const float *T, float *O, int N, int E, t4k_stream_t s);
/* Model::onehot(Dataset&) loss.cpp:47-72: hot[N,E] = 0; hot[n, label<E ? label : 0] = 1 */
int t4k_onehot(const uint32_t *label_dev, float *hot, int N, int E, t4k_stream_t s);
/* Model::hit loss.cpp:75-107: *cnt_dev = sum_n (int)hot[n, argmax_e out[n,e]] (first max wins) */
int t4k_hit(const float *out, const float *hot, int N, int E, int *cnt_dev, t4k_stream_t s);
/* both of the above in one launch (Model::forward on a dataset, forward.cu:57-60: onehot(dset) then hit(true)): hot written from the
   labels, *cnt_dev = number of rows whose first arg-max is the label's class */
int t4k_onehot_hit(const uint32_t *label_dev, float *hot, const float *out, int N, int E, int *cnt_dev, t4k_stream_t s);
/* Dataset::_load dataset.cu:123-158: dst[i] = ((float)src_u8[i] - mean) * scale */
int t4k_u8_normalize(const uint8_t *src_dev, float *dst, long n, float mean, float scale, t4k_stream_t s);
/* Dataset::fetch dataset.cu:64-121 (two host-to-device copies + the _load pass) as ONE launch off device-visible staging memory:
   dst[i] = ((float)src_u8[i] - mean) * scale for i < n, and lab_dst[j] = lab_src[j] for j < nlab (4-byte labels) */
int t4k_stage_batch(const uint8_t *src, float *dst, long n, float mean, float scale,
                    const uint32_t *lab_src, uint32_t *lab_dst, int nlab, t4k_stream_t s);

/* ---------------------------------------------- fused MI355X-native launches */
/* Model::_flinear forward.cu:157-198 in one launch:  Y[N,E0] = X[N,E1] @ W[E0,E1]^T + B[E0] */
int t4k_linear_fwd(const float *X, const float *W, const float *B, float *Y,
                   int N, int E0, int E1, t4k_stream_t s);
/* A run of element-wise layers around one pooling layer, one launch each way (csrc/fused.hip):
 *   X --[pre: dropout | activation]--> pre_out --[pool KSxKS]--> pool_out --[post: activation]--> post_out --[flatten]--> copy_out
 * Absent stages have layer == T4K_L_NONE (KS must be 1 when there is no pooling stage).  The post stage may also be a dropout layer
 * (`leakyrelu dropout`, `maxpool dropout`) when the pre stage is not one: it draws the slice t4k_dropout_mask would draw for post_mask.  Every tensor the
 * separate layers write (_factivate forward.cu:200-209, _fpool :211-227, flatten copy :96) is written with
 * identical values; a dropout pre-stage draws the Philox slice t4k_rand would have drawn for its mask.
 * H0 x W0 is the pooled grid.  On a ceil grid the edge windows are clipped as t4k_pool clips them (max / min over the cells that exist, avg still
 * divides by KS^2).  On a floor grid over an extent that is no multiple of KS some rows / columns belong to no window: the pool stage leaves them alone
 * both ways (the backward keeps the forward values there, as t4k_dpool does), the stages in front of the pool cover their whole tensors. */
typedef struct t4k_poolblock {
    int    pre_layer;  float pre_alpha;  float *pre_mask;  float *pre_out;
    int    pool_layer; int KS;           float *pool_out;
    int    post_layer; float post_alpha; float *post_mask; float *post_out;
    float *copy_out;
} t4k_poolblock;
int t4k_poolblock_fwd(const float *X, const t4k_poolblock *blk, int N, int H1, int W1, int H0, int W0, int C, t4k_stream_t s);
/* the apply half of a batch-norm layer (statistics final in stat_dev, as t4k_batchnorm_fwd leaves them) + such a run right behind it, one pass over the
 * layer's input Y: XH and O (the batch-norm layer's x-hat and output) and every tensor of the run are written exactly as t4k_batchnorm_fwd's apply +
 * t4k_poolblock_fwd(O, ...) would */
int t4k_bn_poolblock_fwd(const float *Y, float *O, float *XH, const float *W, const float *B, const float *stat_dev, const t4k_poolblock *blk,
                         int N, int H1, int W1, int H0, int W0, int C, t4k_stream_t s);
/* convolution + batch norm + such a run (conv -> batchnorm -> [dropout|activation] -> pool -> [activation]): t4k_conv2d_bn_fwd's statistics, then
 * t4k_bn_poolblock_fwd; Hq x Wq = the pooled grid (H0 x W0 when the run has no pool layer) */
int t4k_conv2d_bn_block_fwd(const float *I, float *ICOPY, float *Y, const float *F, const float *Bc,
                            int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P,
                            float *O, float *XH, const float *W, const float *B, float *stat_dev,
                            const t4k_poolblock *blk, int Hq, int Wq, t4k_stream_t s);
/* convolution forward with such a run right behind it (conv -> [dropout|activation] -> 2x2 pool -> [activation] -> [flatten]):
 * O and every tensor of the run are written exactly as t4k_conv2d_fwd2 + t4k_poolblock_fwd would; one launch when the
 * layer takes the gather-MFMA kernel (the pool window is four consecutive accumulator registers of a lane) */
int t4k_conv2d_block_fwd(const float *I, float *ICOPY, float *O, const float *F, const float *B, const t4k_poolblock *blk,
                         int N, int H1, int W1, int C1, int H0, int W0, int C0, int K, int S, int P, t4k_stream_t s);
/* SAMPLE-RESIDENT convolution stack (csrc/conv_stack.hip): 1..3 stages of [conv2d KxK, stride 1, padding K/2 (K = 3 | 5; _fconv
 * forward.cu:115-155, k_conv2d nmath.tcu:34-104) + the element-wise run behind it (t4k_poolblock; 2x2 pool or none)], one workgroup
 * per image with the activations in LDS, ONE launch for the whole stack each way.  Stage s+1 reads the result of stage s's run
 * (H, W of stage s+1 = the pooled grid, C1 = C0 of stage s); only the last run may carry a flatten copy.  Every tensor the separate
 * layers write is written, dropout draws the same Philox slices in layer order.
 * Backward (_bconv backprop.cu:152-191, k_dconv2d nmath.tcu:211-338 incl. its un-flipped dX; _bactivate, _bpool): DY = gradient
 * w.r.t. the last run's last tensor; every run stage's input buffer receives its dX, each conv's input tensor X (forward values on
 * entry) receives dX (`in = dx`) and so does DXS when not NULL; train != 0: DF += sum over the batch, DB likewise (per-image
 * partials in the library workspace, folded in image order by a second small launch - deterministic).
 * t4k_conv_stack_fwd also leaves, per stack, a copy of every conv input and the pool arg-max codes in library memory; a backward that
 * follows it (same N) runs BANDED - several workgroups per image - on those instead of on layer tensors a neighbouring band overwrites in
 * place.  Bit 2 of `train` (train | 4) defers the fold of the dF | dB partials to t4k_opt_step (see there); bit 3 (train | 8) lets the
 * banded kernel skip the dX of stage 0 (t4k_conv_stack_dx0 below).
 * A caller whose latest forward did NOT go through t4k_conv_stack_fwd must say so with bit 1 of `train` (train | 2): the
 * whole-image kernel then reads the layer tensors themselves. */
typedef struct t4k_conv_stage {
    const float *F, *B;       /* filter T4(C1,K,K,C0), bias [C0] */
    float *O;                 /* conv output [N,H,W,C0] */
    float *DF, *DB;           /* backward: parameter gradients (accumulated); unused by the forward */
    float *X, *DXS;           /* backward: the conv's input tensor [N,H,W,C1] and the optional second dX copy */
    int H, W, C1, C0, K;
    t4k_poolblock run;        /* all-zero layers + KS = 1: no run */
} t4k_conv_stage;
int t4k_conv_stack_ok(const t4k_conv_stage *st, int n_stage, int N);           /* 1 when the stack qualifies (shapes, layers, LDS) and its kernels are built */
/* read-only: the launch plan t4k_conv_stack_fwd / _bwd take for this stack and batch - *split = bands per image of the forward, *bsplit = bands
 * of the banded backward (1: whole image per workgroup).  Both follow from N and the CU count (as many bands, <= 4, as give every CU a
 * workgroup while every band keeps a row of every grid and the LDS plan fits).  Returns 1 and fills both, or 0 (nothing written) when the
 * stack does not qualify (t4k_conv_stack_ok == 0). */
int t4k_conv_stack_plan(const t4k_conv_stage *st, int n_stage, int N, int *split, int *bsplit);
/* read-only, no device needed: the preamble the run-time compiled device source is specialised with for this stack at `split` forward and `bsplit`
 * backward bands (1 - 4 each), and the file name of its code object in the disk cache - the hash of preamble + source + options, so two plans that
 * differ in any define never share an object.  Returns 1 and both strings, or 0 when the shapes do not qualify or a buffer is too small. */
int t4k_conv_stack_key(const t4k_conv_stage *st, int n_stage, int split, int bsplit, char *preamble, int preamble_cap, char *name, int name_cap);
int t4k_conv_stack_selftest(void);   /* the stack kernels are compiled at run time (hipRTC) for the model's shapes: this compiles two reference
                                      * shape sets for gfx950 - no device needed - and returns 0, or an error with the compiler log in t4k_last_error() */
/* The stack AND the classifier head behind its flatten in ONE launch: [conv + run] x n, flatten, linear E1 -> E0a, one element-wise layer
 * (dropout / activation, or 0), linear E0a -> E0b, softmax - the layers t4k_conv_stack_fwd + t4k_mlp_head_fwd run (forward.cu:28-113,
 * 157-198, 231-243), every layer tensor stored, Philox positions as the separate layers.  t4k_conv_stack_head_ok() tells whether the shapes
 * qualify; the backward is unchanged (t4k_conv_stack_bwd reads what this forward saved, like t4k_conv_stack_fwd's). */
typedef struct t4k_stack_head {
    const float *W1, *B1; float *Y1;            /* first linear layer: W1[E0a][E1], bias, output [N][E0a]                     */
    int mid_layer; float mid_alpha;             /* element-wise layer behind it (t4k_layer; 0: none), its parameter          */
    float *mid_mask, *mid_out;                  /* derivative mask and output [N][E0a]                                      */
    const float *W2, *B2; float *Y2, *P;        /* second linear layer W2[E0b][E0a], bias, output [N][E0b]; softmax output  */
    int E1, E0a, E0b;
    /* optional (all NULL / 0: off).  The batch came from a dataset: Model::forward then turns the labels into one-hot rows and counts the hits
     * (Model::onehot(Dataset&) loss.cpp:47-72 + hit forward.cu:57-60).  The last band of image n has P[n] in hand: it writes hot[n][0..E0b)
     * (label >= E0b counts as class 0, loss.cpp:66) and hit_flag[n] = (first arg-max of P[n] == label) for n < n_label, 0 behind it - one
     * byte per image in device-visible memory (pinned host memory: the host adds them up, no atomics, no extra launch). */
    const unsigned *label; float *hot; unsigned char *hit_flag; int n_label;
} t4k_stack_head;
/* t4k_conv_stack_release: frees what the forward left behind for the banded backward of the stack whose first conv output tensor is
 * `first_conv_out` (the owner of that tensor calls it when the model is freed - Model::~Model in the reference, src/nn/model.h; unknown
 * keys are ignored).  t4k_conv_stack_stats: how this process got its stack kernels - compiled by hipRTC (*jit), loaded from the
 * code-object cache on disk (*disk: $T4K_CACHE_DIR, <library dir>/kcache as filled by build(), ~/.cache/tensorforth_amd) or not at
 * all (*failed: those stacks run the per-layer kernels; the library says so once on stderr). */
int  t4k_conv_stack_release(const float *first_conv_out);
/* Lazy dX of the FIRST conv layer.  In a classifier's training loop nobody reads the gradient w.r.t. the input batch, yet `in = dx`
 * (backprop.cu:185) makes the reference compute and store it twice per step.  t4k_conv_stack_bwd(train | 8) skips it (banded kernel only)
 * and remembers the filter it belongs to; t4k_conv_stack_dx0_pending() tells the caller whether that happened, t4k_conv_stack_dx0()
 * produces it on demand - X and DXS of stage 0 then hold what the eager backward would have stored (k_dconv2d's dX, nmath.tcu:304-324).
 * The host VM keeps a "stale" mark on the two tensors and calls it before any word can read them (host/tensor.cpp du2obj). */
int  t4k_conv_stack_dx0_pending(const float *first_conv_out);
int  t4k_conv_stack_dx0(const t4k_conv_stage *st, int N, t4k_stream_t s);
void t4k_conv_stack_stats(int *jit, int *disk, int *failed);
int t4k_conv_stack_head_ok(const t4k_conv_stage *st, int n_stage, int N, const t4k_stack_head *h);
int t4k_conv_stack_head_fwd(const float *X, float *X0, const t4k_conv_stage *st, int n_stage, int N, const t4k_stack_head *h, t4k_stream_t s);
int t4k_conv_stack_fwd(const float *X, float *XCOPY, const t4k_conv_stage *st, int n_stage, int N, t4k_stream_t s);
int t4k_conv_stack_bwd(const float *DY, const t4k_conv_stage *st, int n_stage, int N, int train, t4k_stream_t s);
/* 1 when that call would be accepted (kernels built; the banded or the whole-image kernel it would launch fits the LDS and the workspace): the host's
 * quiet test before it picks between the stack's backward and its per-layer kernels */
int t4k_conv_stack_bwd_ok(const t4k_conv_stage *st, int n_stage, int N, int train, t4k_stream_t s);
/* backward of the same run (_bactivate backprop.cu:256-263, _bpool, flatten `in = out`): DY is the gradient
 * w.r.t. the run's last tensor; each stage's input buffer receives its dX (X receives the run's dX). */
int t4k_poolblock_bwd(const float *DY, float *X, const t4k_poolblock *blk, int N, int H1, int W1, int H0, int W0, int C, t4k_stream_t s);
/* linear layer followed by an element-wise layer (t4k_layer: relu ... dropout; _flinear + _factivate forward.cu:157-209):
 * Y as above, ACT_O / ACT_F = activation output / derivative mask of Y; dropout draws the Philox slice t4k_rand would */
int t4k_linear_act_fwd(const float *X, const float *W, const float *B, float *Y, int layer, float alpha,
                       float *ACT_F, float *ACT_O, int N, int E0, int E1, t4k_stream_t s);
/* linear layer + the element-wise run behind it (Model::forward's loop over _flinear, _factivate / dropout, forward.cu:82-209) and,
 * when XCOPY != NULL, the model's copy of the batch into its layer 0 (forward.cu:39: XCOPY[N,E1] = X).  blk (may be NULL) holds the
 * run: pre and/or post stage (any t4k_layer activation or dropout, at most one dropout), no pool, no flatten copy, KS = 1.  Tensors
 * written: Y, each stage's mask and output, XCOPY - the same values as t4k_copy + t4k_linear_fwd + t4k_poolblock_fwd. */
int t4k_linear_block_fwd(const float *X, float *XCOPY, const float *W, const float *B, float *Y, const t4k_poolblock *blk,
                         int N, int E0, int E1, t4k_stream_t s);
/* backward of the same pair, seen from the linear layer behind the run: t4k_linear_bwd(X, W, DY, DX, DW, DB) of a layer whose input X
 * was produced by the element-wise run blk (pre and/or post mask-multiply stage, no pool, KS = 1) followed by that run's backward
 * (t4k_poolblock_bwd(DX, XRUN, blk): the post stage's input buffer = DX * post_mask, XRUN = that * pre_mask; _bactivate
 * backprop.cu:256-263).  TGT != NULL: DY -= TGT first (backprop's start, backprop.cu:43-53), the difference also stored in DY2 when
 * that is not NULL.  DX may alias X (the reference's in-place convention). */
/* Classifier-head backward + the backward of the linear layer in front of it in ONE launch: the two calls
 *   t4k_loss_linear_bwd(X2, W2, P, TGT, Y2, X2, MASK, Y1, DW2, DB2, N, E0b, E0a, 1);   t4k_linear_bwd(X1, W1, Y1, X1, DW1, DB1, N, E0a, E1, 1)
 * (backprop.cu:103-121, 226-254: out -= target, dW2 | dB2, dX2 in place, the mask multiply of the layer between them -> Y1, dW1 | dB1, dX1 over X1),
 * training passes only.  t4k_mlp_head_bwd_ok() says whether the shapes qualify. */
int t4k_mlp_head_bwd_ok(int N, int E1, int E0a, int E0b);
int t4k_mlp_head_bwd(float *X2, const float *W2, float *P, const float *TGT, float *Y2, const float *MASK, float *Y1, float *DW2, float *DB2,
                     float *X1, const float *W1, float *DW1, float *DB1, int N, int E1, int E0a, int E0b, t4k_stream_t s);
/* t4k_mlp_head_bwd with element-wise RUNS of one or two mask-multiply layers (t4k_poolblock, no pool / flatten) instead of the single mask layer:
 * run2 in front of the head layer (XRUN2 = the run's input tensor = the big layer's output), run1 in front of the big layer (NULL: none).
 * train = 0: a frozen net, dX only (gradient tensors may be NULL). */
int t4k_mlp_block_bwd(float *X2, const float *W2, float *P, const float *TGT, float *Y2, const t4k_poolblock *run2, float *XRUN2, float *DW2, float *DB2,
                      float *X1, const float *W1, const t4k_poolblock *run1, float *XRUN1, float *DW1, float *DB1, int N, int E1, int E0a, int E0b, int train, t4k_stream_t s);
int t4k_linear_block_bwd(const float *X, const float *W, float *DY, const float *TGT, float *DY2, float *DX, const t4k_poolblock *blk, float *XRUN,
                         float *DW, float *DB, int N, int E0, int E1, int train, t4k_stream_t s);
/* classifier head in one call: [linear E1 -> H + element-wise layer] + [linear H -> E2 (+ softmax when P2 != NULL)] =
 * t4k_linear_act_fwd(X, W1, B1, Y1, layer, alpha, F1, A1) then t4k_linear_softmax_fwd / t4k_linear_fwd on A1, with every
 * tensor written; when the first GEMM is split along K the second layer's launch folds the slabs itself (one launch fewer) */
int t4k_mlp_head_fwd(const float *X, const float *W1, const float *B1, float *Y1, int layer, float alpha, float *F1, float *A1,
                     const float *W2, const float *B2, float *Y2, float *P2, int N, int H, int E1, int E2, t4k_stream_t s);
/* linear layer followed by a softmax layer (_flinear + _fsoftmax forward.cu:157-198, 229-243): Y as above,
 * P[N,E0] = row softmax of Y; both tensors are written */
int t4k_linear_softmax_fwd(const float *X, const float *W, const float *B, float *Y, float *P,
                           int N, int E0, int E1, t4k_stream_t s);
/* Model::_blinear backprop.cu:193-254: DB += sum dY; DW += dY^T X (if train); DX = dY @ W.
 * DX may alias X's buffer only when the caller guarantees X is no longer needed: the
 * kernels read X for DW before DX is written (stream order).
 * DX == NULL computes dW|dB only, DW == DB == NULL computes dX only. */
int t4k_linear_bwd(const float *X, const float *W, const float *DY, float *DX,
                   float *DW, float *DB, int N, int E0, int E1, int train, t4k_stream_t s);
/* same, plus the backward of a mask-multiply layer (dropout, relu, ...) that sits in front of this linear layer:
 * DXM = DX (*) MASK (`in = out * mask`, _bactivate backprop.cu:256-263); MASK == DXM == NULL behaves as t4k_linear_bwd */
int t4k_linear_bwd2(const float *X, const float *W, const float *DY, float *DX, const float *MASK, float *DXM,
                    float *DW, float *DB, int N, int E0, int E1, int train, t4k_stream_t s);
/* loss-side start of backprop folded into the last linear layer's backward (Model::backprop prep `out -= target`,
 * backprop.cu:60-75, + the pass-through `in = out` of a softmax / sigmoid / log-softmax output layer, :122-131, + _blinear):
 * OUT -= TGT in place, OUT2 = OUT (may be NULL), then exactly t4k_linear_bwd2 with DY = OUT.  One launch when the head is
 * small and DX aliases X; otherwise the separate launches. */
int t4k_loss_linear_bwd(const float *X, const float *W, float *OUT, const float *TGT, float *OUT2, float *DX,
                        const float *MASK, float *DXM, float *DW, float *DB, int N, int E0, int E1, int train, t4k_stream_t s);
/* multi-tensor optimizer step over a parameter table (one launch for all layers).
 * tab_dev: array of n_tensors records {G, DG, M, V, n, Nw} on the device. */
typedef struct { float *G, *DG, *M, *V; long n; int Nw; int pad; } t4k_param_rec;
int t4k_opt_multi(int kind /*0 sgd,1 adam,2 adamw*/, const t4k_param_rec *tab_dev, int n_tensors,
                  long max_n, float lr, float b1, float b2, float wd, t4k_stream_t s);

/* the same step with the launch sized to the parameters (k_opt_multi starts max_n/256 workgroups for EVERY tensor: 8192 waves for the
 * LeNet net's 101 030 parameters).  The caller fills each record's `pad` with the tensor's first 1024-element chunk - the running sum of
 * ceil(n / 1024) over the records before it - and passes the total; one workgroup per chunk. */
int t4k_opt_chunked(int kind, const t4k_param_rec *tab_dev, int n_tensors, int n_chunks,
                    float lr, float b1, float b2, float wd, t4k_stream_t s);
/* Model::sgd / adam / adamw as the host calls them (gradient.cu:63-169): t4k_opt_chunked, plus the work a backward DEFERRED to the
 * optimizer inside the same launch - t4k_conv_stack_bwd(train | 4) leaves its per-workgroup dF | dB partial rows unfolded, and when
 * t4k_opt_step is the next entry point the fold rides in the update (one launch instead of two, bit-identical).  Any OTHER entry point
 * called in between runs the stand-alone fold first, so a caller that reads the gradient tensors, accumulates a second backward or
 * all-reduces the slab before the optimizer sees what the undeferred path leaves.  tab_host: the caller's host copy of tab_dev.
 * The fold rides only when every pending segment is a whole DG tensor of the table (same pointer, same n), tab_host is given, the table has at most
 * 64 records and `s` is the backward's stream; otherwise the stand-alone fold runs first, on the BACKWARD's stream, and the plain step follows on `s`.
 * THE CALLER'S OBLIGATION: call it on the stream of the backward that deferred the fold.  On another stream the fold and the update are two launches on
 * two streams and nothing in the library orders them. */
int t4k_opt_step(int kind, const t4k_param_rec *tab_dev, const t4k_param_rec *tab_host, int n_tensors, int n_chunks,
                 float lr, float b1, float b2, float wd, t4k_stream_t s);
/* the data-parallel form: with the one-shot exchange connected (t4k_xchg_connect, world > 1) every gradient element is summed over all
 * ranks inside the same launch (slab / slab_n: the model's gradient slab, holding every DG of the table); otherwise t4k_opt_step. */
/* One-shot request: the NEXT t4k_opt_chunked / t4k_opt_step / t4k_opt_step_dp on stream order also stores the PRE-update values of the
 * parameter tensor G (a record's G pointer) into G_PREV - the copy rides in the update launch.  Model::backprop defers dX of a first
 * linear layer (`in = dX`, backprop.cu:240, is read by no training loop) and needs the weights of that backward should a word ask for
 * it after the step.  G == NULL cancels a pending request. */
int t4k_opt_snapshot(const float *G, float *G_PREV);
int t4k_opt_snapshot_pending(void);              /* 1 while a request has not been consumed by an optimizer launch (a host checks it after ITS launch) */
int t4k_opt_step_dp(int kind, const t4k_param_rec *tab_dev, const t4k_param_rec *tab_host, int n_tensors, int n_chunks,
                    float lr, float b1, float b2, float wd, float *slab, long slab_n, t4k_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* T4K_H_ */
