/* sputnik-amd C-ABI: the FFI boundary of the block-sparse matmul hot path.
 *
 * Every entry point is extern "C", takes plain structs/pointers/ints and a
 * hipStream_t (passed as void*), and returns a hipError_t value as int
 * (0 == hipSuccess). No torch or C++ types cross this boundary. These are the
 * symbols a ctypes / cgo / JNI binding of the reference's sputnik::block API
 * would bind; INTEGRATION.md shows the bindings.
 *
 * Struct layouts are byte-identical to the C++ descriptors in
 * include/sputnik/block/arguments.h (reference sputnik/block/arguments.h:48-162):
 *   sputnik_block_matrix_t: 88 bytes, fields at 0,4,8,12,16,24,...,72,80
 *   sputnik_matrix_t:       16 bytes, fields at 0,4,8
 *
 * Error behaviour: where the reference aborts (missing transposed-metadata or
 * row-index workspace: dsd_..._tn_align8.cu:73-75, sdd_..._nn_align8.cu:75;
 * no compatible kernel: dsd/cutlass/dsd.cu:68-73) these functions return
 * hipErrorInvalidValue (1) instead; unsupported shapes/block sizes return
 * hipErrorNotSupported (801) exactly as the reference does (dsd.cu:16,
 * block_gemm.h:728-745).
 */
#ifndef SPUTNIK_AMD_H_
#define SPUTNIK_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sputnik_block_matrix {
  int32_t rows;        /* elements */
  int32_t cols;        /* elements */
  int32_t nonzeros;    /* elements = #blocks * block_size^2 */
  int32_t block_size;  /* 16/32/64/128; only 128 is accepted by the ops */
  void *data;          /* #blocks * bs * bs values, block-major, row-major blocks */
  void *offsets;       /* int32[rows/bs + 1] (in blocks) */
  void *indices;       /* int16[#blocks] block-column */
  void *offsets_t;     /* int32[cols/bs + 1] */
  void *indices_t;     /* int16[#blocks] */
  void *block_offsets; /* int32[#blocks] */
  void *row_indices;   /* int16[#blocks] */
  void *bitmask;       /* uint64 BitMatrix words (sputnik_bitmask) */
  uint8_t create_metadata; /* C++ bool */
} sputnik_block_matrix_t;

typedef struct sputnik_matrix {
  int32_t rows;
  int32_t cols;
  void *data;
} sputnik_matrix_t;

enum {
  SPUTNIK_DTYPE_F16 = 0,
  SPUTNIK_DTYPE_BF16 = 1,
};

/* ---- DSD: C = op(A_bcsr) * op(B)   (reference sputnik/block/dsd/dsd.h:10-22) */
int sputnik_dsd(const sputnik_block_matrix_t *a, int transpose_a,
                const sputnik_matrix_t *b, int transpose_b,
                const sputnik_matrix_t *c, int dtype, void *stream);
/* MatmulEx: uses a's precomputed transposed metadata (create_metadata=false). */
int sputnik_dsd_ex(const sputnik_block_matrix_t *a, int transpose_a,
                   const sputnik_matrix_t *b, int transpose_b,
                   const sputnik_matrix_t *c, int dtype, void *stream);

/* ---- DDS: C = op(A) * op(B_bcsr)   (reference sputnik/block/dds/dds.h:10-22) */
int sputnik_dds(const sputnik_matrix_t *a, int transpose_a,
                const sputnik_block_matrix_t *b, int transpose_b,
                const sputnik_matrix_t *c, int dtype, void *stream);
int sputnik_dds_ex(const sputnik_matrix_t *a, int transpose_a,
                   const sputnik_block_matrix_t *b, int transpose_b,
                   const sputnik_matrix_t *c, int dtype, void *stream);

/* ---- Accumulating DSD / DDS: C += op(A) * op(B) (sputnik/block/accumulate.h)
 * C_out = round(acc_fp32 + C_in), rounded once after the add. c_type selects
 * what c->data holds: SPUTNIK_OUT_OPERAND the operands' type (`dtype`),
 * SPUTNIK_OUT_F32 rows x cols floats. Where the sparse operand has no blocks
 * C is neither read nor written; every other element is read and written
 * once. C must not overlap A or B. Always the 8-wave kernel (never the 4-wave
 * kernel, split mode or a transposed-B workspace); otherwise as the plain
 * calls. Any other c_type: hipErrorInvalidValue (1). They never abort. */
enum {
  SPUTNIK_OUT_OPERAND = 0,
  SPUTNIK_OUT_F32 = 1,
};
int sputnik_dsd_acc(const sputnik_block_matrix_t *a, int transpose_a,
                    const sputnik_matrix_t *b, int transpose_b,
                    const sputnik_matrix_t *c, int dtype, int c_type,
                    void *stream);
int sputnik_dsd_ex_acc(const sputnik_block_matrix_t *a, int transpose_a,
                       const sputnik_matrix_t *b, int transpose_b,
                       const sputnik_matrix_t *c, int dtype, int c_type,
                       void *stream);
int sputnik_dds_acc(const sputnik_matrix_t *a, int transpose_a,
                    const sputnik_block_matrix_t *b, int transpose_b,
                    const sputnik_matrix_t *c, int dtype, int c_type,
                    void *stream);
int sputnik_dds_ex_acc(const sputnik_matrix_t *a, int transpose_a,
                       const sputnik_block_matrix_t *b, int transpose_b,
                       const sputnik_matrix_t *c, int dtype, int c_type,
                       void *stream);

/* ---- SDD: C_bcsr = op(A) * op(B) at C's nonzero blocks
 *      (reference sputnik/block/sdd/sdd.h:10-15; needs c->row_indices) */
int sputnik_sdd(const sputnik_matrix_t *a, int transpose_a,
                const sputnik_matrix_t *b, int transpose_b,
                const sputnik_block_matrix_t *c, int dtype, void *stream);

/* ---- SDD with an activation epilogue (sputnik/block/activation.h,
 * INTEGRATION.md 3e). With acc the fp32 accumulator sputnik_sdd would round
 * and T the operand type:
 *   sputnik_sdd_act       Z = round_T(acc), H = round_T(act(float(Z)));
 *                         H -> c->data, Z -> z when z != NULL
 *   sputnik_sdd_act_grad  c->data = round_T(float(round_T(acc)) *
 *                         act'(float(Z))), Z read from z (required)
 * z holds c->nonzeros elements of T in c's storage order and must not overlap
 * c->data, A or B. act: SPUTNIK_ACT_RELU, SPUTNIK_ACT_GELU (the tanh form)
 * or SPUTNIK_ACT_SILU, evaluated in fp32 (formulas in activation.h); every
 * finite Z gives a finite result, NaN / inf in Z what the fp32 formula
 * yields. Two routes give the same bits: the 8-wave kernel's fused epilogue,
 * or sputnik_sdd as it stands followed by the elementwise kernel below (knob
 * "sdd_act_route"). `ws`, `ws_bytes`: as sputnik_sdd_ws (used on the
 * two-kernel route only; the fused route never takes the transposed-B path,
 * and sputnik_sdd_workspace_bytes answers as for sputnik_sdd).
 * They never abort: an unknown act, a null operand, a null z in the grad
 * form, or z == c->data: hipErrorInvalidValue (1); block size != 128:
 * hipErrorNotSupported; a shape sputnik_sdd rejects is rejected the same
 * way. */
enum {
  SPUTNIK_ACT_RELU = 0,
  SPUTNIK_ACT_GELU = 1,
  SPUTNIK_ACT_SILU = 2,
};
int sputnik_sdd_act(const sputnik_matrix_t *a, int transpose_a,
                    const sputnik_matrix_t *b, int transpose_b,
                    const sputnik_block_matrix_t *c, int act, void *z,
                    int dtype, void *ws, size_t ws_bytes, void *stream);
int sputnik_sdd_act_grad(const sputnik_matrix_t *a, int transpose_a,
                         const sputnik_matrix_t *b, int transpose_b,
                         const sputnik_block_matrix_t *c, int act,
                         const void *z, int dtype, void *ws, size_t ws_bytes,
                         void *stream);
/* The elementwise stage alone, over n elements of block data (dtype 0 fp16,
 * 1 bf16): h[i] = round_T(act(float(z[i]))), and the gate
 * out[i] = round_T(float(g[i]) * act'(float(z[i]))). h may be z, out may be
 * g or z (in place). 16-byte accesses when every buffer is 16-byte aligned.
 * hipErrorInvalidValue for an unknown act or dtype, n < 0, or a null buffer
 * with n > 0. */
int sputnik_block_activation(const void *z, void *h, long long n, int act,
                             int dtype, void *stream);
int sputnik_block_activation_grad(const void *g, const void *z, void *out,
                                  long long n, int act, int dtype,
                                  void *stream);
/* Diagnostic: the route sputnik_sdd_act[_grad] would take for this problem
 * now, 1 = fused, 2 = two kernels, -1 = rejected. */
int sputnik_sdd_act_route(const sputnik_matrix_t *a, int transpose_a,
                          const sputnik_matrix_t *b, int transpose_b,
                          const sputnik_block_matrix_t *c);

/* ---- SDD with a gated (GLU) epilogue (sputnik/block/gated.h,
 * INTEGRATION.md 3f). With acc the fp32 accumulator sputnik_sdd would round
 * and T the operand type:
 *   sputnik_sdd_gated       U = round_T(acc),
 *                           H = round_T(float(U) * act(float(G)));
 *                           H -> c->data, U -> up when up != NULL,
 *                           G read from gate (required)
 *   sputnik_sdd_gated_grad  D = round_T(acc),
 *                           up_grad = round_T(float(D) * act(float(G))),
 *                           c->data = round_T((float(D) * float(U)) *
 *                           act'(float(G))); G read from gate, U from up,
 *                           all three required
 * gate, up and up_grad hold c->nonzeros elements of T in c's storage order.
 * up_grad may be exactly up (in place); otherwise none of gate, up, up_grad,
 * c->data, A, B may overlap. act, the routes, the knob "sdd_act_route",
 * sputnik_sdd_act_route, `ws` and `ws_bytes`: as sputnik_sdd_act.
 * They never abort: an unknown act, a null operand, a null required buffer,
 * or a buffer that equals one it must not overlap: hipErrorInvalidValue (1),
 * nothing launched; block size != 128: hipErrorNotSupported; a shape
 * sputnik_sdd rejects is rejected the same way. */
int sputnik_sdd_gated(const sputnik_matrix_t *a, int transpose_a,
                      const sputnik_matrix_t *b, int transpose_b,
                      const sputnik_block_matrix_t *c, int act,
                      const void *gate, void *up, int dtype, void *ws,
                      size_t ws_bytes, void *stream);
int sputnik_sdd_gated_grad(const sputnik_matrix_t *a, int transpose_a,
                           const sputnik_matrix_t *b, int transpose_b,
                           const sputnik_block_matrix_t *c, int act,
                           const void *gate, const void *up, void *up_grad,
                           int dtype, void *ws, size_t ws_bytes, void *stream);
/* The elementwise stages alone, over n elements of block data (dtype 0 fp16,
 * 1 bf16): out[i] = round_T(float(u[i]) * act(float(g[i]))), and the pair
 * du[i] = round_T(float(d[i]) * act(float(g[i]))), dg[i] = round_T((float(d[i])
 * * float(u[i])) * act'(float(g[i]))). out may be u or g, dg may be d, du may
 * be u (in place). 16-byte accesses when every buffer is 16-byte aligned.
 * hipErrorInvalidValue for an unknown act or dtype, n < 0, a null buffer
 * with n > 0, or dg == du. */
int sputnik_block_gate(const void *u, const void *g, void *out, long long n,
                       int act, int dtype, void *stream);
int sputnik_block_gate_grad(const void *d, const void *g, const void *u,
                            void *dg, void *du, long long n, int act,
                            int dtype, void *stream);

/* ---- SDD with a column bias, column sums (sputnik/block/bias.h,
 * INTEGRATION.md 3i). bias: c->cols elements of T indexed by C's logical
 * column, any 2-byte alignment. With x = round_T(acc),
 *   xb = round_T((float(x) + float(bias[col])) + 0.0f)
 * and the product sees xb where the bias-free one sees x:
 *   sputnik_sdd_bias        c->data = xb
 *   sputnik_sdd_bias_act    as sputnik_sdd_act on xb; z (may be NULL)
 *                           receives xb
 *   sputnik_sdd_bias_gated  as sputnik_sdd_gated on xb; up (may be NULL)
 *                           receives xb
 * The gradient products read the kept z / up as they stand. A bias that is
 * NULL or equals c->data, z / gate / up, A or B: hipErrorInvalidValue, nothing
 * launched. Routes, workspace arguments and acceptance as sputnik_sdd_act.
 *   sputnik_block_column_sum  out[c] = sum_r float(s[r, c]) over the stored
 *                           blocks, fp32 [s->cols]; +0 for a column block
 *                           without blocks; no atomics, no workspace, same
 *                           bits on every run. Needs s->offsets_t and
 *                           s->block_offsets (NULL: hipErrorInvalidValue). */
int sputnik_sdd_bias(const sputnik_matrix_t *a, int transpose_a,
                     const sputnik_matrix_t *b, int transpose_b,
                     const sputnik_block_matrix_t *c, const void *bias,
                     int dtype, void *ws, size_t ws_bytes, void *stream);
int sputnik_sdd_bias_act(const sputnik_matrix_t *a, int transpose_a,
                         const sputnik_matrix_t *b, int transpose_b,
                         const sputnik_block_matrix_t *c, const void *bias,
                         int act, void *z, int dtype, void *ws,
                         size_t ws_bytes, void *stream);
int sputnik_sdd_bias_gated(const sputnik_matrix_t *a, int transpose_a,
                           const sputnik_matrix_t *b, int transpose_b,
                           const sputnik_block_matrix_t *c, const void *bias,
                           int act, const void *gate, void *up, int dtype,
                           void *ws, size_t ws_bytes, void *stream);
int sputnik_block_column_sum(const sputnik_block_matrix_t *s, int dtype,
                             float *out, void *stream);

/* ---- Caller-owned workspaces for the transposed-B path
 * SDD NT / TT, and DSD NT over a nearly dense A, transpose B once into a
 * scratch buffer when B is at least "sdd_bt_min_mib" MiB and the product is
 * dense enough, then run the N-major kernel. There are two routes.
 *
 * Library route (nothing supplied; the behaviour of earlier versions): the
 * buffer is the library's, one per (device, stream). It is allocated inside
 * the first such product, grown with a stream synchronize and a free when a
 * larger B arrives, and kept until sputnik_release_workspaces(). A stream
 * being captured, and hipStreamPerThread, keep the NT / TT kernel.
 *
 * Caller route: the caller supplies the memory, per call (the _ws entry
 * points) or per stream (sputnik_set_stream_workspace). Such a product
 * allocates, frees and synchronises nothing (sputnik_incall_events does not
 * move), takes no library lock across the launch, and enqueues the same two
 * launches eagerly, while `stream` is being captured, and on
 * hipStreamPerThread. Memory that is smaller than the query below asks for,
 * or not 16-byte aligned, keeps the NT / TT kernel for that product; it never
 * falls back to the library's buffer.
 *
 * Lifetime: the memory must stay valid until all work enqueued with it has
 * finished, and for a captured launch until the graph and every executable
 * made from it are destroyed. A graph that captured it must not replay
 * concurrently with other work that uses the same memory. */
/* Bytes the transposed copy takes for this problem under the current knobs,
 * rounded up to 256; 0 when the path does not apply (the product then needs
 * no workspace). Host-only: ignores capture state, allocates and launches
 * nothing. */
size_t sputnik_sdd_workspace_bytes(const sputnik_matrix_t *a, int transpose_a,
                                   const sputnik_matrix_t *b, int transpose_b,
                                   const sputnik_block_matrix_t *c);
size_t sputnik_dsd_workspace_bytes(const sputnik_block_matrix_t *a,
                                   int transpose_a, const sputnik_matrix_t *b,
                                   int transpose_b, const sputnik_matrix_t *c);
/* Per-call route: sputnik_sdd / sputnik_dsd / sputnik_dsd_ex with `ws_bytes`
 * bytes of device memory at `ws`. ws == NULL or ws_bytes == 0 means no
 * workspace: exactly the plain entry point. */
int sputnik_sdd_ws(const sputnik_matrix_t *a, int transpose_a,
                   const sputnik_matrix_t *b, int transpose_b,
                   const sputnik_block_matrix_t *c, int dtype, void *ws,
                   size_t ws_bytes, void *stream);
int sputnik_dsd_ws(const sputnik_block_matrix_t *a, int transpose_a,
                   const sputnik_matrix_t *b, int transpose_b,
                   const sputnik_matrix_t *c, int dtype, void *ws,
                   size_t ws_bytes, void *stream);
int sputnik_dsd_ex_ws(const sputnik_block_matrix_t *a, int transpose_a,
                      const sputnik_matrix_t *b, int transpose_b,
                      const sputnik_matrix_t *c, int dtype, void *ws,
                      size_t ws_bytes, void *stream);
/* Per-stream route, for callers bound to the reference's fixed signatures
 * (the C++ Matmul / MatmulEx, and the plain entry points above): registers
 * `bytes` of device memory at `ptr` for (current device, stream); ptr == NULL
 * unregisters. The plain entry points look the registration up under a short
 * lock, released before anything is enqueued, and then run the caller route;
 * a stream with a registration never uses the library's buffer.
 * hipErrorInvalidValue (1) for a pointer that is not 16-byte aligned, for
 * bytes == 0 with a non-null pointer, and for hipStreamPerThread (one handle,
 * a different stream in every thread); hipErrorOutOfMemory (2) when all 16
 * entries are taken. */
int sputnik_set_stream_workspace(void *stream, void *ptr, size_t bytes);
/* Device memory the library holds on the current device: transposed-B
 * buffers, eager and capture pair-balancing workspaces, persistent tile
 * counters. Host-only query. */
size_t sputnik_retained_bytes(void);
/* Synchronises the current device, frees every library-owned transposed-B
 * buffer on it and returns the bytes freed; a later product on the library
 * route allocates again. Pair workspaces and tile counters are not touched
 * (sputnik_capture_workspaces returns the captured ones). */
size_t sputnik_release_workspaces(void);
/* Two process-wide counters that only grow. incall_events: every hipMalloc,
 * hipFree, hipStreamSynchronize and hipDeviceSynchronize the library executed
 * inside a product call (the transposed-B buffer, pair workspaces, tile
 * counters). bt_launches: every transpose of B enqueued for a product, by
 * either route, eager or captured. */
unsigned long long sputnik_incall_events(void);
unsigned long long sputnik_bt_launches(void);

/* ---- SSD: C_bcsr = op(A_bcsr) * op(B) at C's nonzero blocks
 *      (reference sputnik/block/ssd/ssd.h:10-22; needs c->row_indices, and
 *      a's transposed metadata when transpose_a) */
int sputnik_ssd(const sputnik_block_matrix_t *a, int transpose_a,
                const sputnik_matrix_t *b, int transpose_b,
                const sputnik_block_matrix_t *c, int dtype, void *stream);
int sputnik_ssd_ex(const sputnik_block_matrix_t *a, int transpose_a,
                   const sputnik_matrix_t *b, int transpose_b,
                   const sputnik_block_matrix_t *c, int dtype, void *stream);

/* ---- SDS: C_bcsr = op(A) * op(B_bcsr) at C's nonzero blocks
 *      (reference sputnik/block/sds/sds.h:10-22; needs c->row_indices, and
 *      b's transposed metadata when !transpose_b) */
int sputnik_sds(const sputnik_matrix_t *a, int transpose_a,
                const sputnik_block_matrix_t *b, int transpose_b,
                const sputnik_block_matrix_t *c, int dtype, void *stream);
int sputnik_sds_ex(const sputnik_matrix_t *a, int transpose_a,
                   const sputnik_block_matrix_t *b, int transpose_b,
                   const sputnik_block_matrix_t *c, int dtype, void *stream);

/* ---- DSS: C = op(A_bcsr) * op(B_bcsr), dense
 *      (reference sputnik/block/dss/dss.h:10-22; K <= 32768; a's transposed
 *      metadata when transpose_a, b's when !transpose_b; no bitmask needed) */
int sputnik_dss(const sputnik_block_matrix_t *a, int transpose_a,
                const sputnik_block_matrix_t *b, int transpose_b,
                const sputnik_matrix_t *c, int dtype, void *stream);
int sputnik_dss_ex(const sputnik_block_matrix_t *a, int transpose_a,
                   const sputnik_block_matrix_t *b, int transpose_b,
                   const sputnik_matrix_t *c, int dtype, void *stream);

/* ---- Metadata builders */
/* reference sputnik/block/row_indices/row_indices.h:10 */
int sputnik_row_indices(const sputnik_block_matrix_t *a, int16_t *row_indices,
                        void *stream);
/* reference sputnik/block/transpose/transpose.h:10 (device, bit-identical) */
int sputnik_transpose(const sputnik_block_matrix_t *a, void *stream);

/* reference sputnik/block/bitmask/bitmask.h:10 (device, bit-identical
 * BitMatrix layout: rows of ceil(cols/64) uint64 words). Orientation as the
 * reference: over the transposed order when m->offsets_t is set. */
int sputnik_bitmask(const sputnik_block_matrix_t *m, void *stream);
/* Bytes of m's bitmask workspace (reference AllocateBitmaskBuffers,
 * bitmask.h:16-23; host-only). */
size_t sputnik_bitmask_bytes(const sputnik_block_matrix_t *m);

/* ---- Device topology builders (no host round trip) */
/* Block mask (uint8 [block_rows][block_cols] row-major, nonzero = present)
 * -> BCSR offsets int32[block_rows+1] and ascending int16 indices, the
 * reference's mask -> CSR scan (sputnik/matrix_utils.cu:254-289, pad_rows_to
 * = 1). `indices` must hold the mask's nonzero count (block_rows*block_cols
 * bounds it); block_cols <= 32768. */
int sputnik_mask_to_bcsr(const uint8_t *mask, int block_rows, int block_cols,
                         int32_t *offsets, int16_t *indices, void *stream);
/* MegaBlocks dMoE topology: padded_bins int32[num_experts] = cumulative
 * per-expert token counts, each padded to a multiple of 128. Block-row r
 * belongs to expert e = #{e : padded_bins[e] <= 128 r} (clamped to the last
 * expert) and holds block-columns [e*blocks_per_expert, (e+1)*...).
 * offsets int32[block_rows+1], indices int16[block_rows*blocks_per_expert]. */
int sputnik_expert_topology(const int32_t *padded_bins, int num_experts,
                            int block_rows, int blocks_per_expert,
                            int32_t *offsets, int16_t *indices, void *stream);

/* ---- MoE token permutation (sputnik/block/moe.h): the
 * counterparts of MegaBlocks' padded_gather, padded_scatter and
 * padded_scatter_wgrad, and the routing metadata behind them. With T the
 * operand type, n = tokens * top_k assignments (assignment a = t * top_k + k)
 * and the int32 routing tensors of MegaBlocks' indices_and_padded_bins
 * (bin_ids, indices: the stable ascending sort of top_experts.flatten();
 * bins / padded_bins: inclusive cumsums of the per-expert counts / of the
 * counts rounded up to multiples of 128; all of num_experts entries):
 *   sputnik_moe_bins        bins, tokens_per_expert, padded_bins from the
 *                           sorted bin_ids[n] (one workgroup; the sort is
 *                           the caller's)
 *   sputnik_moe_row_map     row_of[indices[i]] = padded_bins[e-1] +
 *                           (i - bins[e-1]), e = bin_ids[i] (index -1 read
 *                           as 0): the padded row of every assignment; -1
 *                           where the bin id is outside [0, num_experts) or
 *                           the row outside [0, rows); a position whose
 *                           index is outside [0, n) is skipped
 *   sputnik_padded_gather   x [tokens, hidden] -> out [rows, hidden]:
 *                           out[row(i)] = x[indices[i] / top_k] bit for bit,
 *                           or round_T(float(w[indices[i]]) * float(x[..]))
 *                           with weights; every other row of out (padding
 *                           inside a bin, rows from padded_bins[E-1] to
 *                           rows) is written as +0 by the same kernel: out
 *                           needs no initialisation
 *   sputnik_padded_scatter  y [rows, hidden] -> out [tokens, hidden]:
 *                           out[t] = round_T(sum_k float(w[t top_k + k]) *
 *                           float(y[row_of[t top_k + k]])), summed in fp32
 *                           from 0 in ascending k, rounded once; no
 *                           atomics, no [n, hidden] intermediate, bitwise
 *                           reproducible
 *   sputnik_padded_scatter_wgrad
 *                           dw[a] = sum_h float(dout[a / top_k, h]) *
 *                           float(y[row_of[a], h]), fp32 accumulation in a
 *                           free order, stored in the weights' type
 * weights: n elements indexed by assignment, of T (weights_dtype
 * SPUTNIK_WEIGHTS_OPERAND) or float (SPUTNIK_WEIGHTS_F32); NULL means
 * unweighted (weights_dtype is then ignored). dw is of weights_dtype. The
 * gradients are these same calls: d gather / dx is the unweighted scatter,
 * d scatter / dy the gather of dout with the weights, d scatter / dw the
 * wgrad. Every index read from device memory is range-checked before it is
 * used as an address; an entry out of range contributes zeros, so no kernel
 * reads or writes outside its buffers whatever the metadata holds. 16-byte
 * accesses when hidden % 8 == 0 and the row buffers are 16-byte aligned.
 * Stream-ordered; no call allocates or synchronises.
 * They never abort: a null required buffer, a negative size, top_k < 1,
 * rows % 128 != 0, an unknown dtype or weights_dtype, tokens * top_k or
 * n + 127 * num_experts past INT_MAX, or an output that equals an input:
 * hipErrorInvalidValue (1), nothing launched. Zero-sized work (no output
 * element) succeeds whatever the pointers. */
enum {
  SPUTNIK_WEIGHTS_OPERAND = 0,
  SPUTNIK_WEIGHTS_F32 = 1,
};
int sputnik_moe_bins(const int32_t *bin_ids, int n, int num_experts,
                     int32_t *bins, int32_t *tokens_per_expert,
                     int32_t *padded_bins, void *stream);
int sputnik_moe_row_map(const int32_t *indices, const int32_t *bin_ids,
                        const int32_t *bins, const int32_t *padded_bins,
                        int n, int num_experts, int rows, int32_t *row_of,
                        void *stream);
int sputnik_padded_gather(const void *x, const int32_t *indices,
                          const int32_t *bins, const int32_t *padded_bins,
                          const void *weights, void *out, int tokens,
                          int hidden, int top_k, int num_experts, int rows,
                          int dtype, int weights_dtype, void *stream);
int sputnik_padded_scatter(const void *y, const int32_t *row_of,
                           const void *weights, void *out, int tokens,
                           int hidden, int top_k, int rows, int dtype,
                           int weights_dtype, void *stream);
int sputnik_padded_scatter_wgrad(const void *dout, const void *y,
                                 const int32_t *row_of, void *dw, int tokens,
                                 int hidden, int top_k, int rows, int dtype,
                                 int weights_dtype, void *stream);

/* The scatter with an output bias [num_experts, hidden] of T (moe.h
 * PaddedScatterBias*): out[t] = round_T(sum_k w_k * (float(y[row_k]) +
 * float(bias[e_k]))), one fp32 add, multiply and accumulate per k, e_k read
 * off the row through padded_bins; a row outside [0, rows) or past the last
 * padded bin contributes zero, bias included. _wgrad: dw[a] = sum_h dout *
 * (y + bias). _grad: bias_grad[e, h] = sum over e's sorted positions of
 * w * dout, fp32 [num_experts, hidden], no atomics, no workspace, same bits
 * on every run, +0 for an expert without tokens. Argument rules as above. */
int sputnik_padded_scatter_bias(const void *y, const int32_t *row_of,
                                const int32_t *padded_bins, const void *bias,
                                const void *weights, void *out, int tokens,
                                int hidden, int top_k, int num_experts,
                                int rows, int dtype, int weights_dtype,
                                void *stream);
int sputnik_padded_scatter_bias_wgrad(const void *dout, const void *y,
                                      const int32_t *row_of,
                                      const int32_t *padded_bins,
                                      const void *bias, void *dw, int tokens,
                                      int hidden, int top_k, int num_experts,
                                      int rows, int dtype, int weights_dtype,
                                      void *stream);
int sputnik_padded_scatter_bias_grad(const void *dout, const int32_t *indices,
                                     const int32_t *bins, const void *weights,
                                     float *bias_grad, int tokens, int hidden,
                                     int top_k, int num_experts, int dtype,
                                     int weights_dtype, void *stream);

/* ---- MoE router and device sort (sputnik/block/router.h, INTEGRATION.md
 * 3h): what stands in front of the permutation above. L is the logits' type
 * (logits_dtype SPUTNIK_ROUTER_F16 / _BF16 / _F32), W the type of weights,
 * scores and their gradients: L (SPUTNIK_WEIGHTS_OPERAND) or float
 * (SPUTNIK_WEIGHTS_F32).
 *   sputnik_router_topk       logits L [tokens, E] -> top_experts int32
 *                             [tokens, top_k], weights W [tokens, top_k] and,
 *                             with scores != NULL, scores W [tokens, E]. The
 *                             picks are the top_k largest logits in
 *                             descending order, equal values to the lower
 *                             index, NaN below -inf: always top_k distinct
 *                             ids in [0, E). fp32 arithmetic: p = softmax of
 *                             the row (max subtracted), weights = p at the
 *                             picks, divided by their sum with normalize;
 *                             each output rounded once.
 *   sputnik_router_topk_grad  dlogits L [tokens, E] from logits, top_experts,
 *                             dweights W [tokens, top_k] and an optional
 *                             dscores W [tokens, E] (NULL: zero); the softmax
 *                             is recomputed. An id outside [0, E)
 *                             contributes nothing, a duplicated id twice.
 *   sputnik_moe_sort          top_experts.flatten() int32 [n] -> indices,
 *                             bin_ids [n], bins, tokens_per_expert,
 *                             padded_bins [E], row_of [n]: a stable counting
 *                             sort in three launches, for ids in [0, E)
 *                             bit-identical to a stable sort + moe_bins +
 *                             moe_row_map. An id out of range: no bin, row_of
 *                             -1, sorted behind bins[E-1] with bin_ids = E.
 *                             workspace: sputnik_moe_sort_workspace_bytes(n,
 *                             E) = ceil(n / 1024) * (E + 1) * 4 bytes, no
 *                             initialisation needed.
 * 1 <= E <= 1024, 1 <= top_k <= min(E, 32), rows % 128 == 0. Every id read
 * from device memory is range-checked before it forms an address.
 * Stream-ordered; no call allocates, synchronises or aborts: a null required
 * buffer, a size outside the limits, an unknown type, n + 127 E past INT_MAX,
 * a workspace too small or an output equal to an input or another output:
 * hipErrorInvalidValue (1), nothing launched. Zero-sized work succeeds. */
enum {
  SPUTNIK_ROUTER_F16 = 0,
  SPUTNIK_ROUTER_BF16 = 1,
  SPUTNIK_ROUTER_F32 = 2,
};
int sputnik_router_topk(const void *logits, int32_t *top_experts,
                        void *weights, void *scores, int tokens,
                        int num_experts, int top_k, int normalize,
                        int logits_dtype, int weights_dtype, void *stream);
int sputnik_router_topk_grad(const void *logits, const int32_t *top_experts,
                             const void *dweights, const void *dscores,
                             void *dlogits, int tokens, int num_experts,
                             int top_k, int normalize, int logits_dtype,
                             int weights_dtype, void *stream);
/* The router with the statistics of the auxiliary losses (RouterTopKAux /
 * RouterTopKAuxGrad in sputnik/block/router.h): the ids, weights and scores
 * of sputnik_router_topk bit for bit, plus score_sums float [E] (required) =
 * sum_t p_te and z_sum float [1] (optional) = sum_t (log sum_j exp l_tj)^2,
 * fp32 from the unrounded values, without atomics: a function of the input
 * alone. workspace: sputnik_router_aux_workspace_bytes(tokens, E) =
 * ceil(tokens / 64) * (E + 1) * 4 bytes, 4-byte aligned, no initialisation
 * needed; tokens = 0 needs none and still writes the zeros. The gradient
 * takes dscore_sums float [E] and dz_sum float [1] (a device pointer), either
 * may be NULL; with both NULL it is sputnik_router_topk_grad bit for bit. */
size_t sputnik_router_aux_workspace_bytes(int tokens, int num_experts);
int sputnik_router_topk_aux(const void *logits, int32_t *top_experts,
                            void *weights, void *scores, float *score_sums,
                            float *z_sum, int tokens, int num_experts,
                            int top_k, int normalize, int logits_dtype,
                            int weights_dtype, void *workspace,
                            size_t workspace_bytes, void *stream);
int sputnik_router_topk_aux_grad(const void *logits,
                                 const int32_t *top_experts,
                                 const void *dweights, const void *dscores,
                                 const float *dscore_sums, const float *dz_sum,
                                 void *dlogits, int tokens, int num_experts,
                                 int top_k, int normalize, int logits_dtype,
                                 int weights_dtype, void *stream);
/* The router with sigmoid scores, a selection bias and a group-limited
 * choice (RouterScoreTopK / RouterScoreTopKGrad in sputnik/block/router.h):
 * s = 1 / (1 + exp(-logit)); the picks are the top_k largest s + bias (bias
 * float [E], NULL: 0) among the experts of the topk_groups best of num_groups
 * groups, a group's score being the sum of its two largest s + bias; weights
 * = s at the picks, divided by their sum with normalize, times scale; scores
 * (optional) = s. Ties to the lower index, NaN last: always top_k distinct
 * ids in [0, E). 1 <= topk_groups <= num_groups <= 64, E % num_groups == 0,
 * top_k <= min(32, topk_groups * E / num_groups), scale finite. The gradient
 * recomputes s and takes neither bias nor groups. */
int sputnik_router_score_topk(const void *logits, const float *bias,
                              int32_t *top_experts, void *weights,
                              void *scores, int tokens, int num_experts,
                              int top_k, int num_groups, int topk_groups,
                              int normalize, float scale, int logits_dtype,
                              int weights_dtype, void *stream);
int sputnik_router_score_topk_grad(const void *logits,
                                   const int32_t *top_experts,
                                   const void *dweights, const void *dscores,
                                   void *dlogits, int tokens, int num_experts,
                                   int top_k, int normalize, float scale,
                                   int logits_dtype, int weights_dtype,
                                   void *stream);
size_t sputnik_moe_sort_workspace_bytes(int n, int num_experts);
int sputnik_moe_sort(const int32_t *top_experts, int n, int num_experts,
                     int rows, int32_t *indices, int32_t *bin_ids,
                     int32_t *bins, int32_t *tokens_per_expert,
                     int32_t *padded_bins, int32_t *row_of, void *workspace,
                     size_t workspace_bytes, void *stream);

/* ---- FP8 (e4m3) expert products with block scales, forward
 * (sputnik/block/fp8.h has the contract, INTEGRATION.md 3j the recipe).
 * Elements are OCP e4m3fn bytes (torch.float8_e4m3fn), scales fp32 with
 * value = float(q) * scale: one per 1 x 128 row tile of an activation or of
 * a sparse operand's stored blocks, one per 128 x 128 weight block.
 * scale = max(amax / 448, 2^-126), or with `pow2` the smallest power of two
 * >= 2^-126 with amax / scale <= 448; q = rne_e4m3(x / scale), both IEEE
 * fp32 divisions; NaN / +-Inf become 0x7F / 0xFF.
 *
 *   sputnik_quantize_rows        x [rows, cols] of T -> q [rows, cols],
 *                                scales [rows, cols / 128]
 *   sputnik_quantize_rows_act    the same of round_T(act(x)), as
 *                                sputnik_block_activation computes it
 *   sputnik_quantize_rows_gated  the same of round_T(x * act(gate)), as
 *                                sputnik_block_gate computes it
 *   sputnik_quantize_weight      w [k, n] of T (transpose: the buffer is
 *                                [n, k]) -> q [n, k], scales [k / 128, n / 128]
 *   sputnik_sdd_fp8   C (BCSR, T) = Aq [c.rows, k] . Bq at C's stored blocks
 *                     (c.indices and c.row_indices); a_scales [c.rows,
 *                     k / 128], Bq [c.cols, k], b_scales [k / 128,
 *                     c.cols / 128]
 *   sputnik_dsd_fp8   C [s.rows, c.cols] (T) = Sq (BCSR, e4m3 bytes in
 *                     s.data, s_scales [blocks * 128]) . Bq [c.cols, s.cols]
 *
 * Per k-block in ascending (SDD) or storage (DSD) order, acc = fma(sa * sb, P,
 * acc) in fp32 with P the MFMA sum of the block's 128 products, held to fp32
 * precision; C = round_T(acc).
 * No split-K, no atomics: bitwise reproducible. `dtype` is T (0 fp16,
 * 1 bf16), act 0 relu / 1 gelu / 2 silu. Stream-ordered; nothing is
 * allocated or synchronised. hipErrorInvalidValue with nothing launched for
 * a null required buffer, a negative size, a dimension that is not a multiple
 * of 128, an output that is one of the inputs, or (the two products) a
 * 16-byte misaligned Aq / Sq / Bq / C. Zero-sized work succeeds. */
int sputnik_quantize_rows(const void *x, int rows, int cols, void *q,
                          float *scales, int pow2, int dtype, void *stream);
int sputnik_quantize_rows_act(const void *x, int rows, int cols, int act,
                              void *q, float *scales, int pow2, int dtype,
                              void *stream);
int sputnik_quantize_rows_gated(const void *x, const void *gate, int rows,
                                int cols, int act, void *q, float *scales,
                                int pow2, int dtype, void *stream);
int sputnik_quantize_weight(const void *w, int k, int n, int transpose,
                            void *q, float *scales, int pow2, int dtype,
                            void *stream);
int sputnik_sdd_fp8(const void *aq, const float *a_scales, int k,
                    const void *bq, const float *b_scales,
                    const sputnik_block_matrix_t *c, int dtype, void *stream);
int sputnik_dsd_fp8(const sputnik_block_matrix_t *s, const float *s_scales,
                    const void *bq, const float *b_scales,
                    const sputnik_matrix_t *c, int dtype, void *stream);
/* The two products with the accumulation mode of P (Fp8Accumulate in
 * sputnik/block/fp8.h): `accumulate` 0 is the fp32 sum of the entry points
 * above, bit for bit; 1 is the opt-in fast mode, where P is what one
 * v_mfma_scale_f32_16x16x128_f8f6f4 returns for the interval (unit scales,
 * from +0; fp8.h has the lane assignment, the error bound with its measured
 * eps_fast and the NaN rule). Any other value: hipErrorInvalidValue, nothing
 * launched. sputnik_fp8_interval_sums writes that P itself, fp32 [k / 128, m,
 * n], of aq [m, k] and bq [n, k] (m, n, k multiples of 128; aq, bq, p
 * non-null, 16-byte aligned, p none of the inputs): a cold kernel, the
 * definition the fast products are tested against. */
int sputnik_sdd_fp8_acc(const void *aq, const float *a_scales, int k,
                        const void *bq, const float *b_scales,
                        const sputnik_block_matrix_t *c, int dtype,
                        int accumulate, void *stream);
int sputnik_dsd_fp8_acc(const sputnik_block_matrix_t *s, const float *s_scales,
                        const void *bq, const float *b_scales,
                        const sputnik_matrix_t *c, int dtype, int accumulate,
                        void *stream);
int sputnik_fp8_interval_sums(const void *aq, const void *bq, int m, int n,
                              int k, int accumulate, float *p, void *stream);
/* The gradients' pieces (sputnik/block/fp8.h, "Gradients", has the contract
 * and the table of the backward pass).
 *
 *   sputnik_quantize_tiles   x [rows, cols] of T, both multiples of 128 ->
 *                            the row outputs of sputnik_quantize_rows (q,
 *                            scales) and / or the column outputs qt [cols,
 *                            rows], scales_t [rows / 128, cols], one scale
 *                            per 128 x 1 column tile. A pair may be null.
 *   sputnik_quantize_blocks  the block values of s after `stage` (0 none,
 *                            1 act(x), 2 x * act'(z)): row outputs in
 *                            storage order (q, scales [blocks * 128]) and /
 *                            or column outputs in the transposed order of
 *                            s.block_offsets (qt: output block j is source
 *                            block block_offsets[j] transposed; scales_t
 *                            [blocks * 128], one per source column)
 *   sputnik_fp8_transpose_weight
 *                            q [n, k], scales [k / 128, n / 128] -> qt
 *                            [k, n], scales_t [n / 128, k / 128], exact
 *   sputnik_dsd_fp8_wgrad    sputnik_dsd_fp8_acc with b_scales [s.cols /
 *                            128, c.cols], one per interval and column:
 *                            acc = fma(sa[row] * sb[kb, col], P, acc). `out`
 *                            0: C of T, 1: C of fp32; `add`: C = round(acc +
 *                            float(C)), and block rows of s without blocks
 *                            are left untouched. */
int sputnik_quantize_tiles(const void *x, int rows, int cols, void *q,
                           float *scales, void *qt, float *scales_t, int pow2,
                           int dtype, void *stream);
int sputnik_quantize_blocks(const sputnik_block_matrix_t *s, int stage,
                            int act, const void *z, void *q, float *scales,
                            void *qt, float *scales_t, int pow2, int dtype,
                            void *stream);
int sputnik_fp8_transpose_weight(const void *q, const float *scales, int k,
                                 int n, void *qt, float *scales_t,
                                 void *stream);
int sputnik_dsd_fp8_wgrad(const sputnik_block_matrix_t *s,
                          const float *s_scales, const void *bq,
                          const float *b_scales, const sputnik_matrix_t *c,
                          int dtype, int out, int add, int accumulate,
                          void *stream);

/* ---- Host-only queries (no GPU work; safe without a device) */
/* 1 when the reference would accept the problem (same rules as
 * can_launch_* + ValidMatmul), 0 otherwise. op: 0=DSD 1=DDS 2=SDD. */
int sputnik_can_implement(int op, const void *a, int transpose_a,
                          const void *b, int transpose_b, const void *c);
/* sizeof / offsetof of the descriptors, for ABI checks by bindings. */
size_t sputnik_abi_block_matrix_size(void);
size_t sputnik_abi_block_matrix_offset(int field);
size_t sputnik_abi_matrix_size(void);
const char *sputnik_version(void);
/* Hash of the sources the library was built from (bench.py compares it
 * with the tree it runs in). */
const char *sputnik_build_hash(void);

/* ---- Diagnostics (need a device) */
/* SDD tile plan: 1 = grouped 128x512 tiles (>= 4 blocks per CU), 2 = the
 * grouped tiles with each group's K split over 2-8 workgroups (SDD NN, few
 * groups: one workgroup per CU), 0 = one k-split 128x128 block per
 * workgroup, -1 = the problem is rejected. (Decides as a launch on the null
 * stream would, allocating nothing.) */
int sputnik_sdd_plan(const sputnik_matrix_t *a, int transpose_a,
                     const sputnik_matrix_t *b, int transpose_b,
                     const sputnik_block_matrix_t *c);
/* The SDD kernel behind that plan: 0 = the 8-wave k-split block tile,
 * 1 = grouped tiles on the 8-wave kernel, 2 = the 4-wave K-split, 3 =
 * grouped tiles on the 4-wave kernel, 4 = (NT / TT over a B past the
 * MALL) B transposed into a scratch buffer, then grouped tiles on the
 * 4-wave kernel, -1 = rejected. Answers for an eager launch on the null
 * stream with no workspace registered; under capture, code 4 needs a
 * caller-owned workspace (the _ws entry points or
 * sputnik_set_stream_workspace) -- without one a captured launch runs 3. */
int sputnik_sdd_kernel(const sputnik_matrix_t *a, int transpose_a,
                       const sputnik_matrix_t *b, int transpose_b,
                       const sputnik_block_matrix_t *c);
/* DDS kernel plan of a problem launched on `stream` (no launch, nothing
 * allocated): 0 = the 8-wave 128x512 tile, 1 = the 4-wave kernel, 2 = the
 * tall configuration, 3 = split mode (8-wave), -1 = rejected. */
int sputnik_dds_plan(const sputnik_matrix_t *a, int transpose_a,
                     const sputnik_block_matrix_t *b, int transpose_b,
                     const sputnik_matrix_t *c, hipStream_t stream);
/* DSD kernel plan of a problem launched on `stream` (no launch; makes the
 * launch's workspace decisions): 0 = the 8-wave 128x512 tile, 1 = the
 * 4-wave hand-scheduled kernel, 2 = the tall configuration, 3 = split mode,
 * 4 = the tall pipeline (4-wave, persistent, NN), -1 = the problem is
 * rejected. */
int sputnik_dsd_plan(const sputnik_block_matrix_t *a, int transpose_a,
                     const sputnik_matrix_t *b, int transpose_b,
                     const sputnik_matrix_t *c, hipStream_t stream);
/* Number of pair hand-offs on the current device whose consumer workgroup
 * timed out waiting for its partial (a bounded 0.2 s wait) since the last
 * call; such a consumer's output tile is written as NaN, never as a partial
 * sum. Callers that share the GPU with other work can poll this after a
 * launch to detect the (otherwise unobserved) event. Clears the counts.
 * Synchronizes the device. -1 on a HIP error. */
int sputnik_pair_errors(void);
/* Workspaces made for launches captured into graphs on the current device
 * (pair-balancing workspaces + persistent tile counters). A captured launch
 * gets one per (capture, capturing stream). Once the captured graph and
 * every executable made from it are destroyed, its workspace is re-used by
 * the next capture that needs one, and this call frees the ones still
 * unused (the only place the library frees them: no free ever runs inside
 * a launch). A graph must not be replayed concurrently with a second
 * instantiation of the same capture. Host-only query. */
int sputnik_capture_workspaces(void);

/* ---- Test hooks and tuning knobs: UNSUPPORTED.
 * For the library's own tests and same-process A/B experiments; a correct
 * caller never needs them, names and ranges may change between versions,
 * and every setting is process-wide. */
/* Test hook: when on, pair producers never publish (forces the timeout).
 * Same as sputnik_tuning_set("pair_fault", on). */
void sputnik_debug_pair_fault(int on);
/* Kernel choice for DSD / DDS (every transpose) and the grouped SDD: 1 =
 * the 4-wave hand-scheduled kernel where it applies and pays (the default),
 * 2..7 = wherever it applies, whatever the density, with the DSD NN variant
 * kEpi = mode - 2 (0 workgroup epilogue, 1 per-wave, 2 per-wave +
 * specialized last block, 3 double slots, 4 double slots + barrier every
 * other step + interleaved copy-out, 5 double slots + interleaved copy-out;
 * DDS NN runs kEpi 1 for modes 2-4 and kEpi 3 for 5-7, the grouped SDD the
 * barrier-every-other-step variant for mode 6 and double slots otherwise,
 * the transposed DSD / DDS launches the one variant they have), 0 = the
 * 8-wave kernel everywhere, -1 = query only. Returns the previous choice.
 * Same as the knob "dsd4w". */
int sputnik_select_dsd_kernel(int four_wave);
/* Tuning knobs, each initialised from its environment variable
 * SPUTNIK_AMD_<NAME> (upper case) or its default: "pairs" (1), "pair_xcd2"
 * (3), "split" (1), "split_min_bn" (128), "dsd4w" (1), "grouped_sdd" (1),
 * "grouped_min_per_cu" (4), "tall" (1), "tall_persistent" (1), "dds_xcd2"
 * (3), "sdd4w_max_ld" (16384), "pair_fault" (0), "sdd_ksplit" (1: off;
 * 2-8 the most K-split chunks -- its chunks wait on each other, so only
 * where the launch has the device to itself),
 * "sdd_ksplit_min_k" (6144), "sdd_order" (1),
 * "tall4w" (1: the tall DSD NN pipeline), "tall_flush_w" (4: a tile
 * store's weight in quarter blocks for the pipeline's work split),
 * "tall_odd_share" (120: an odd XCD's workgroup share in percent of an even
 * one's), "sdd_act_route" (0: auto -- the SDD activation products run fused
 * where the plain SDD would run the 8-wave kernel, as two kernels otherwise;
 * 1 fused, 2 two kernels; same results either way).
 * An environment value that does not parse or is out of range
 * means the default. get returns the value,
 * set the previous value; both return INT_MIN for an unknown name, set also
 * for a value out of the knob's range (nothing changes then). */
int sputnik_tuning_get(const char *name);
int sputnik_tuning_set(const char *name, int value);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif  /* SPUTNIK_AMD_H_ */
