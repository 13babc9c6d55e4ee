/*
 * gcn_spmm.h — C-ABI of the MI355X (gfx950) GraphConvolution hot path.
 *
 * This is the drop-in boundary for the sparse x dense products of LinChen-65/pygcn's
 * GraphConvolution layer.  The reference has no FFI of its own for this path: it calls PyTorch,
 *
 *     output = torch.spmm(adj, support)              pygcn/layers.py:34     (forward,  A · B)
 *     grad_support = adj.t() @ grad_output           torch autograd `mm` mat2 formula, triggered
 *                                                    by loss.backward() at pygcn/train.py:157
 *     output + self.bias                             pygcn/layers.py:35-36  (fused epilogue)
 *
 * so the entry points below are what a binding for those three lines has to call.  Plain
 * pointers and sizes only — no torch types.  Every `const void*`/pointer marked DEVICE must be
 * hipMalloc'ed memory of the current device; the launchers never allocate, never synchronise
 * and enqueue on the stream they are given (so they are hipGraph-capturable).  The planner
 * entry points (`*_host`) are pure CPU code on HOST arrays.
 *
 * Return value of every function: 0 on success, a hipError_t (> 0) for HIP failures,
 * a negative GCN_E_* for argument errors.  gcn_last_error() gives a message.
 */
#ifndef GCN_SPMM_H
#define GCN_SPMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCN_E_BADARG   (-1)   /* null pointer / negative size / inconsistent plan            */
#define GCN_E_ALIGN    (-2)   /* (reserved) alignment the selected kernel cannot handle       */
#define GCN_E_WORKSPACE (-3)  /* workspace smaller than gcn_spmm_workspace_bytes()            */
#define GCN_E_CAPACITY (-4)   /* planner output arrays too small                              */

#define GCN_DTYPE_F32  0      /* B, C fp32; fp32 accumulate  (configs C1-C4)                  */
#define GCN_DTYPE_BF16 1      /* B, C bf16 storage; fp32 values and accumulate (config C5)    */

#define GCN_ABI_VERSION 26

#define GCN_DEFAULT_ITEM_COST   64     /* work units (stored entries + rows) per row-batch item */
#define GCN_DEFAULT_LONG_THRESH 256    /* rows with more stored entries are chunked             */

/*
 * A CSR adjacency (or its transpose) plus the static launch schedule built for it once.
 * All pointers are DEVICE pointers.  The schedule splits the rows of the matrix into
 *   - row-batch items : runs of <= 64 consecutive "short" rows whose stored entries are
 *                       contiguous; one wavefront streams one item;
 *   - long rows       : rows with more than `long_thresh` stored entries, cut into chunks of
 *                       `long_thresh` entries that are summed by separate wavefronts into a
 *                       partial slab and then added in chunk order (bitwise reproducible;
 *                       no float atomics).
 * Replaces: the torch sparse tensor `adj` the reference builds at pygcn/utils.py:407-414 and
 * passes to GraphConvolution.forward (pygcn/layers.py:32).
 */
typedef struct gcn_csr_plan {
    int64_t n_rows;
    int64_t n_cols;
    int64_t nnz;
    const void *rowptr;        /* [n_rows+1] int32 or int64                                  */
    int32_t rowptr_is64;
    int32_t long_thresh;       /* chunk length L for long rows                               */
    const int32_t *col;        /* [nnz] column index of every stored entry                   */
    const float *val;          /* [nnz] fp32 value of every stored entry                     */
    int64_t n_items;
    const int32_t *items;      /* [2*n_items] (first_row, end_row) per row-batch item        */
    int64_t n_chunks;
    const int32_t *chunk_row;  /* [n_chunks] row every chunk belongs to                      */
    const int64_t *chunk_e0;   /* [n_chunks] first stored entry of the chunk                 */
    int64_t n_long;
    const int32_t *long_row;   /* [n_long] row index of every long row                       */
    const int32_t *long_chunk0;/* [n_long+1] first chunk of every long row                   */
} gcn_csr_plan;

/* ABI history: 21 = round 2's surface.  26: the ReLU + BatchNorm sweeps gcn_bn_workspace_bytes / gcn_bn_stats /
 * gcn_bn_apply / gcn_bn_backward_sums / gcn_bn_backward_apply — new entry points only; nothing existing changed.
 * Additive to 26 (the number did not move: a library without them fails to bind with a message naming the
 * missing symbol): the column-window forms gcn_bn_batched_workspace_bytes / gcn_bn_stats_batched /
 * gcn_bn_apply_batched / gcn_bn_backward_sums_batched / gcn_bn_backward_apply_batched for k samples side by
 * side (the fork's per-sample loop, reference pygcn/models.py:343-349) and the masked mean pool
 * gcn_pool_workspace_bytes / gcn_masked_colsum / gcn_masked_broadcast (its PoolLayer, reference
 * pygcn/models.py:267-286); the existing gcn_bn_ entry points are now the batch = 1 launch of the same kernels,
 * with the same results.  Also additive to 26: the vertex-attention sweeps gcn_attn_workspace_bytes /
 * gcn_attn_scores / gcn_attn_normalize / gcn_attn_backward (the head of its SoftGenerator, reference
 * pygcn/models.py:324-329).  Also additive to 26: vertex selection, gcn_select_workspace_bytes / gcn_select_kth /
 * gcn_select_indices / gcn_topk_flag / gcn_race_keys (the end of its Generator, Hierarchical_Generator and of
 * SoftGenerator's policy step, reference pygcn/models.py:373-377, rl-policy-generator.py:324-336).  Also additive to
 * 26: the input side of its evaluator, gcn_eval_workspace_bytes / gcn_eval_ingest / gcn_eval_ingest_backward
 * (GCN_OVER_MLP and PoolLayer, reference pygcn/models.py:333-355, :267-286).  Also additive to 26: gcn_dropout_rows /
 * gcn_csr_take_rows (dropout keyed by a row list and row blocks of a CSR matrix, for the forward pass restricted
 * to the loss rows' receptive field).  Also additive to 26: gcn_bn_linear_workspace_bytes / gcn_bn_linear_forward /
 * gcn_bn_linear_backward_sums / gcn_bn_linear_backward_apply (ReLU + BatchNorm folded into the next layer's X·W for
 * 32-wide layers).  Also additive to 26: gcn_agg_linear_partial_rows / gcn_agg_linear_forward /
 * gcn_agg_linear_backward (the dense half of an aggregate-first input layer, (A·X)·W + b, for inputs of 4 .. 32
 * columns into a 32-wide layer).  Also additive to 26: gcn_csr_sample_rows, at most K stored entries per row of a
 * CSR matrix (neighbour sampling).
 * 25 (round 4, late): new entry point gcn_gemm_atg256_f32_b3_colsum (the
 * weight gradient with the bias gradient Σ G[rows] as a side result); gcn_gemm_atg256_workspace_bytes grew by
 * 1 KiB per workgroup; struct gcn_gemm_epilogue gained keep_bits_out / mask_bits at its END (zero them);
 * nothing else changed.  24 (round 4): new entry points gcn_gemm_xw256_f32_b3 /
 * gcn_gemm_atg256_f32_b3 (the fp32-EQUIVALENT three-part bf16 form of the 256-wide GEMMs with the
 * full option set of the _h2 entry points: row lists, forward epilogue, backward mask, max|Y|) and
 * gcn_gemm_xw256_b3_workspace_bytes; nothing existing changed.  23 (round 3, late): at p = 1/2 the dropout keep function
 * draws 128 one-bit fields per Philox call (other p unchanged) — masks at p = 1/2 differ from ABI
 * 22's; no signature or struct changed.  22 (round 3): the dropout keep function draws eight 16-bit
 * fields per Philox call instead of four 32-bit words and takes a row base (drop_row_base in both
 * epilogue structs) and the product can report max|result| (gcn_epilogue.c_absmax); new entry
 * points gcn_nll_log_softmax_backward_colsum, gcn_gemm_atg_bf16, gcn_sddmm_csr, gcn_rows_pack_count /
 * gcn_rows_pack_values / gcn_rows_unpack / gcn_bits_row_counts; gcn_gemm_xw_bf16
 * takes a backward mask.  The three options that leave
 * rows of an output unwritten (c_skip_zero_rows, c_row_select, skip_zero_rows of the backward
 * sweeps) are EXPERIMENTAL: the product uses them only inside single autograd nodes that own both
 * the producer and every consumer of such a tensor (pygcn_amd/fused.py). */
/* ABI version of the loaded library (GCN_ABI_VERSION). */
int gcn_abi_version(void);

/* Message for the last non-zero return on this thread. */
const char *gcn_last_error(void);

/*
 * Planner, pass 1: count items / chunks / long rows for a HOST rowptr.
 *   item_cost   : target work per row-batch item, in units of (stored entries + rows); <= 0
 *                 selects GCN_DEFAULT_ITEM_COST.
 *   long_thresh : rows with more stored entries than this are chunked; <= 0 selects the
 *                 GCN_DEFAULT_LONG_THRESH.
 */
int gcn_plan_count_host(const void *rowptr_host, int rowptr_is64, int64_t n_rows,
                        int32_t item_cost, int32_t long_thresh, int64_t *n_items,
                        int64_t *n_chunks, int64_t *n_long);

/*
 * Planner, pass 2: fill caller-allocated HOST arrays (sizes from pass 1):
 *   items[2*n_items], chunk_row[n_chunks], chunk_e0[n_chunks], long_row[n_long],
 *   long_chunk0[n_long+1].  The caller copies them to the device and points a gcn_csr_plan
 *   at the copies.  items and long_chunk0 are never NULL; chunk_row / chunk_e0 may be NULL only
 *   with n_chunks == 0 and long_row only with n_long == 0 (GCN_E_BADARG otherwise).
 */
int gcn_plan_fill_host(const void *rowptr_host, int rowptr_is64, int64_t n_rows,
                       int32_t item_cost, int32_t long_thresh, int32_t *items, int64_t n_items,
                       int32_t *chunk_row, int64_t *chunk_e0, int64_t n_chunks,
                       int32_t *long_row, int32_t *long_chunk0, int64_t n_long);

/*
 * The same planner ON THE DEVICE: rowptr is a DEVICE array and never visits
 * the host; the result equals gcn_plan_{count,fill}_host array for array.  Two calls around one
 * 24-byte read:
 *   gcn_plan_count_device  computes the schedule into `workspace` and writes
 *                          counts[0..2] = (n_items, n_chunks, n_long) to DEVICE memory;
 *   (the caller copies the three counts to the host and allocates the plan arrays on the device)
 *   gcn_plan_fill_device   writes items[2*n_items], chunk_row[n_chunks], chunk_e0[n_chunks],
 *                          long_row[n_long], long_chunk0[n_long+1] (DEVICE arrays) from the
 *                          workspace gcn_plan_count_device left behind (same stream / ordered).
 * Greedy segmentation in parallel: per-row item ends by binary search in scanned row costs, item
 * starts by pointer doubling over "next item start" (pygcn_amd/csrc/gcn_plan.hip).  Scratch:
 * gcn_plan_device_workspace_bytes(n_rows) (48 B per row + scan temporaries).
 */
size_t gcn_plan_device_workspace_bytes(int64_t n_rows);
int gcn_plan_count_device(const void *rowptr, int rowptr_is64, int64_t n_rows, int32_t item_cost,
                          int32_t long_thresh, void *workspace, size_t workspace_bytes,
                          int64_t *counts, void *stream);
int gcn_plan_fill_device(const void *rowptr, int rowptr_is64, int64_t n_rows, int32_t long_thresh,
                         const void *workspace, size_t workspace_bytes, int32_t *items,
                         int64_t n_items, int32_t *chunk_row, int64_t *chunk_e0, int64_t n_chunks,
                         int32_t *long_row, int32_t *long_chunk0, int64_t n_long, void *stream);

/* Bytes of DEVICE scratch gcn_spmm_csr() needs for feature width F (0 if no long rows). */
size_t gcn_spmm_workspace_bytes(const gcn_csr_plan *plan, int64_t F);

/*
 * C[n_rows, F] = A · B  (+ bias[F], then ReLU, both optional) on `stream`.
 *
 *   plan       : the CSR matrix A [n_rows, n_cols] and its schedule.
 *   dtype      : GCN_DTYPE_F32 or GCN_DTYPE_BF16 (element type of B and C).
 *   B          : DEVICE [n_cols, F] row-major with leading dimension ldb (elements).
 *   C          : DEVICE [n_rows, F] row-major with leading dimension ldc (elements);
 *                every row is written (rows without stored entries become bias / zero).
 *   bias       : DEVICE fp32 [F] or NULL                      — pygcn/layers.py:35-36.
 *   relu       : non-zero applies max(x, 0) after the bias    — pygcn/models.py:48 (upstream).
 *   workspace  : DEVICE scratch of at least gcn_spmm_workspace_bytes(plan, F) bytes
 *                (may be NULL when that is 0).
 *
 * Forward of pygcn/layers.py:34 when `plan` describes adj; the backward product
 * adj.t() @ grad_output when `plan` describes CSR(adj^T) (see gcn_csr_transpose_*).
 */
int gcn_spmm_csr(const gcn_csr_plan *plan, int dtype, const void *B, int64_t ldb, void *C,
                 int64_t ldc, int64_t F, const float *bias, int relu, void *workspace,
                 size_t workspace_bytes, void *stream);

/*
 * Epilogue applied to every output row inside the kernel's store, in this order:
 *   x = acc + bias[f]            (bias may be NULL)          — pygcn/layers.py:35-36
 *   x = max(x, 0)                if relu                     — F.relu,   pygcn/models.py:48 (upstream)
 *   x = keep ? x * s : 0         if dropout_p > 0            — F.dropout, pygcn/models.py:50 (upstream)
 * The keep bit of element (row, f) is a pure function of (seed, drop_row_base + row, f), identical
 * for every kernel variant.  T = clamp(round(p * 65536), 1, 65535) (p is honoured to 2^-17; p = 1/2
 * exactly); s = 65536 / (65536 - T) = 1 / (keep probability of that T) (ABI 24; before: 1 / (1 - p) of
 * the unquantised p), so E[dropout(x)] = x exactly — the backward scale of a caller must be the
 * same number (pygcn_amd.spmm.dropout_scale); w = Philox4x32-10(counter = (row_lo, row_hi, block, 0), key = (seed_lo, seed_hi)), and
 *   T != 32768 (ABI 22: eight 16-bit fields per call):
 *     block = ((f >> 4) << 1) | ((f >> 2) & 1),   field = (((f >> 3) & 1) << 2) | (f & 3)
 *     keep  = ((w[field >> 1] >> 16 * (field & 1)) & 0xFFFF) >= T
 *   T == 32768, i.e. p = 1/2 — one bit decides (ABI 23: 128 one-bit fields per call):
 *     block = ((f >> 8) << 1) | ((f >> 2) & 1),   index = (((f & 255) >> 3) << 2) | (f & 3)
 *     keep  = (w[index >> 5] >> (index & 31)) & 1
 * Because out > 0 <=> (pre-activation > 0 and kept), no mask is stored: the backward pass is
 * gcn_relu_dropout_backward on the output itself.
 */
typedef struct gcn_epilogue {
    const float *bias;   /* DEVICE fp32 [F] or NULL */
    int32_t relu;
    float dropout_p;     /* in [0, 1); 0 disables dropout */
    uint64_t seed;
    /* Optional hint about the dense operand B (both NULL = none): bit c of the bitmap
     * b_row_nonzero[ceil(n_cols/32)] is clear for rows of B that are entirely zero, *b_nnz_rows
     * counts the rows whose bit is set.  Such rows are
     * not gathered (their products are zero anyway, so the result is unchanged up to summation
     * order); the hint is ignored on the device when it cannot pay (3/4 or more of the rows
     * non-zero for rows of >= 528 bytes, 1/8 or more for narrower rows).  Produced for free by
     * gcn_relu_dropout_backward_colsum — the gradients of a semi-supervised loss
     * (`nll_loss(output[idx_train], ...)`, pygcn/train.py) are non-zero on few rows. */
    const uint32_t *b_row_nonzero;
    const int32_t *b_nnz_rows;
    /* Optional second block of the dense operand (NULL = B is one block): rows b_split, b_split+1,
     * ... of B are read from b2 (row-major, leading dimension ldb2, same dtype) instead.  Lets the
     * sharded path multiply with [own activation rows | received halo rows] without copying the
     * own rows next to the halo buffer. */
    const void *b2;
    int64_t ldb2;
    int64_t b_split;
    /* Optional OUTPUT (NULL = none): byte flags [n_rows], zeroed by the caller; c_row_nonzero[r]
     * is set to 1 where row r of the stored result has a non-zero element.  Lets the consumer of a
     * row-sparse product (the weight / input gradient GEMMs behind A^T · grad) skip the zero rows
     * without another pass over the result. */
    uint8_t *c_row_nonzero;
    /* Non-zero: store log_softmax over each row of (A·B + bias) instead of the row itself — the
     * `F.log_softmax(x, dim=1)` that ends the reference model (pygcn/models.py:52 upstream).
     * The row must live in one wavefront's store: F <= 64 elements, or F a multiple of the 16-byte
     * lane width v (4 fp32 / 8 bf16) with F/v <= 64 and 16-byte aligned operands; not combinable
     * with relu / dropout.  Backward: gcn_log_softmax_backward_colsum. */
    int32_t log_softmax;
    /* Optional DEVICE pointer to the dropout seed (NULL: use `seed`).  The kernel reads the seed
     * when it runs, not when it is enqueued, so a launch captured into a hipGraph draws a fresh
     * mask on every replay if the graph also updates *seed_dev (e.g. a captured increment). */
    const uint64_t *seed_dev;
    /* Optional bitmap over the OUTPUT rows (NULL = all rows wanted): rows whose bit in
     * c_row_select[ceil(n_rows/32)] is clear are not needed by the caller — the kernel may skip
     * their stored entries and leave those rows of C unwritten (contents undefined).  Lets
     * grad_W = (A·X)^T · grad of a first layer be formed from the rows of A·X that meet a non-zero
     * row of grad only (the bitmap gcn_relu_dropout_backward_colsum already produced). */
    const uint32_t *c_row_select;
    /* With c_row_nonzero: rows of the result that are entirely zero are NOT stored (their flag
     * stays 0, their memory is left untouched) — for a consumer that reads the flagged rows only.
     * Rows longer than the plan's long_thresh are always stored. */
    int32_t c_skip_zero_rows;
    /* Added to the row index in the dropout counter (ABI 22): a row-block shard passes the global
     * index of its first row, so the masks of a sharded run are those of the single-GPU run. */
    int64_t drop_row_base;
    /* Optional OUTPUT (NULL = none; ABI 22): one DEVICE float, zeroed by the caller, that receives
     * max |stored value| of the launch (atomic max of the bit patterns: inf / NaN patterns sort
     * above every finite value, so an overflow is never lost) — the bound the scaled GEMMs that
     * consume this product need (gcn_gemm_xw256_f32_h2: x_absmax_bound), without a reduction pass
     * over the result.  One atomic per wavefront at most. */
    float *c_absmax;
} gcn_epilogue;

/* gcn_spmm_csr with the full epilogue (ep may be NULL: plain product). */
int gcn_spmm_csr_ep(const gcn_csr_plan *plan, int dtype, const void *B, int64_t ldb, void *C,
                    int64_t ldc, int64_t F, const gcn_epilogue *ep, void *workspace,
                    size_t workspace_bytes, void *stream);

/*
 * grad_pre[i] = out[i] > 0 ? grad_out[i] * scale : 0 over n_elems contiguous elements
 * (scale = 1 / (1 - p); 1 for a bare ReLU).  DEVICE pointers; grad_pre may alias grad_out.
 * Backward of the fused epilogue above (autograd of F.relu + F.dropout in the reference model).
 */
int gcn_relu_dropout_backward(int dtype, const void *grad_out, const void *out, void *grad_pre,
                              int64_t n_elems, float scale, void *stream);

/*
 * The same backward pass for fp32 or bf16 [n_rows, F] row-major tensors (`dtype`; colsum is always
 * fp32 and, for bf16, sums the rounded values that were stored), producing in the same sweep the
 * column sums of its result: colsum[f] = sum_rows grad_pre[row, f] — the bias gradient of
 * `output + self.bias` (pygcn/layers.py:35-36).  `out == NULL` skips the masking (plain column
 * sums of grad_out; grad_pre is then ignored).  Deterministic (per-block partial rows added in
 * block order, no float atomics).  F must be a multiple of the 16-byte lane width v (4 fp32 / 8
 * bf16) with F/v dividing 256; scratch: gcn_bwd_colsum_workspace_bytes(n_rows, F, dtype).
 * Optional outputs (both or neither; F/v <= 64, GCN_E_BADARG for wider rows — they are never
 * silently left unwritten): bit r of row_bits[ceil(n_rows/32)] is set where
 * row r of the result has a non-zero element, *nnz_rows = how many — the B-operand hint of
 * gcn_epilogue.  skip_zero_rows != 0 (needs those outputs and `out`): rows of the result that are
 * entirely zero are NOT written to grad_pre — for a consumer that reads the flagged rows only
 * (the hinted product below 3/4 resp. 1/8 non-zero rows, the row-compacted GEMMs); at a 5 %
 * labelled share that removes 95 % of the pass's writes.
 */
size_t gcn_bwd_colsum_workspace_bytes(int64_t n_rows, int64_t F, int dtype);
/*
 * Backward of the fused log_softmax epilogue with the same by-products: out = log_softmax(z) row
 * by row, grad_pre = grad_out - exp(out) * rowsum(grad_out), colsum[f] = sum_rows grad_pre[row, f],
 * and the row bitmap / count of grad_pre.  Rows of grad_out that are entirely zero (every vertex
 * outside idx_train) give zero rows without `out` being read.  Same shape rules and scratch as
 * gcn_relu_dropout_backward_colsum, with F/v <= 64 required (a row inside one wavefront).
 */
int gcn_log_softmax_backward_colsum(int dtype, const void *grad_out, const void *out, void *grad_pre,
                                    float *colsum, int64_t n_rows, int64_t F, uint32_t *row_bits,
                                    int32_t *nnz_rows, int skip_zero_rows, void *workspace,
                                    size_t workspace_bytes, void *stream);
int gcn_relu_dropout_backward_colsum(int dtype, const void *grad_out, const void *out, void *grad_pre,
                                     float *colsum, int64_t n_rows, int64_t F, float scale,
                                     uint32_t *row_bits, int32_t *nnz_rows, int skip_zero_rows,
                                     void *workspace, size_t workspace_bytes, void *stream);
/*
 * The same sweep for the gradient of a MEAN NLL LOSS OVER ALL ROWS — `F.nll_loss(output, labels)`,
 * the reference's loss line (pygcn/train.py:153) without its index selection; the fork's live
 * loss likewise reduces over every vertex (pygcn/train.py:151-155).  That gradient has one
 * non-zero per row, grad_out[r][target[r]] = *coef (coef = -upstream / n_rows, DEVICE float), so it
 * is never materialised: grad_pre = *coef * (onehot(target[r]) - exp(out[r])) and its column sums
 * come straight from `out` (log-probabilities, [n_rows, F]) and the label vector `target` (DEVICE
 * int64 [n_rows], entries in [0, F); a NEGATIVE entry marks an ignored row — torch's ignore_index =
 * -100 — whose gradient row is zero; the caller's coef then divides by the rows that count).
 * 2 full-height streams (read out, write grad_pre) instead of 4.  Shape rules and scratch of
 * gcn_log_softmax_backward_colsum.  (ABI 22.)
 */
int gcn_nll_log_softmax_backward_colsum(int dtype, const int64_t *target, const float *coef,
                                        const void *out, void *grad_pre, float *colsum, int64_t n_rows,
                                        int64_t F, void *workspace, size_t workspace_bytes, void *stream);

/*
 * SDDMM on the pattern of `plan`: out_vals[e] = < G[row(e), :], B[col[e], :] > for every stored
 * entry e (fp32 results; G [n_rows, F] and B [n_cols, F] row-major fp32 or bf16, leading dimensions
 * in elements).  The gradient of the adjacency VALUES for a caller that sets adj.requires_grad —
 * PyTorch's `mm` derivative for a sparse first operand, (grad · mat2^T) sampled on self's pattern;
 * the reference never needs it (its adj is a constant: pygcn/train.py:80,123), SURVEY row f4 lists
 * it as optional.  Uses the schedule of `plan` (items, long-row chunks); no workspace, no atomics,
 * deterministic.  (ABI 22.)
 */
int gcn_sddmm_csr(const gcn_csr_plan *plan, int dtype, const void *G, int64_t ldg, const void *B,
                  int64_t ldb, int64_t F, float *out_vals, void *stream);

/*
 * CSR(A^T) on the HOST from CSR(A) on the HOST: stable counting sort by column, so each row of
 * A^T lists its entries in increasing source-row order (deterministic backward sums).
 * rowptr_t[n_cols+1] has the width of rowptr; col_t[nnz]; val_t[nnz].
 */
int gcn_csr_transpose_host(const void *rowptr_host, int rowptr_is64, const int32_t *col,
                           const float *val, int64_t n_rows, int64_t n_cols, void *rowptr_t,
                           int32_t *col_t, float *val_t);

/*
 * Device-side ingest — everything below runs on `stream`, never allocates.
 *
 * gcn_csr_transpose_device: CSR(A) -> CSR(A^T) entirely on the DEVICE (stable radix sort by
 * column carrying (source row, value)); each row of A^T lists its entries in increasing
 * source-row order, exactly like gcn_csr_transpose_host.  All array arguments are DEVICE
 * pointers; rowptr_t has the width of rowptr.  Scratch: gcn_csr_transpose_workspace_bytes().
 * Replaces the transposed view PyTorch re-derives on every backward call of torch.spmm
 * (autograd of pygcn/layers.py:34).
 */
size_t gcn_csr_transpose_workspace_bytes(int64_t n_rows, int64_t n_cols, int64_t nnz);
int gcn_csr_transpose_device(const void *rowptr, int rowptr_is64, const int32_t *col,
                             const float *val, int64_t n_rows, int64_t n_cols, int64_t nnz,
                             void *rowptr_t, int32_t *col_t, float *val_t, void *workspace,
                             size_t workspace_bytes, void *stream);

/*
 * COO -> CSR on the DEVICE with duplicate reduction: the adjacency construction of the reference's
 * data recipe (pygcn/utils.py:360-368: scipy `coo_matrix(...)`, symmetrization, `+ I`) and of
 * `sparse_mx_to_torch_sparse_tensor` consumers (utils.py:407-414: int64 [2, nnz] indices, fp32
 * values, uncoalesced).  Entries may come in any order; entries with the same (row, col) are
 * reduced IN STORAGE ORDER with
 *   GCN_REDUCE_SUM  what scipy's coo->csr conversion and torch.spmm on an uncoalesced tensor do;
 *   GCN_REDUCE_MAX  elementwise maximum — `adj + adj.T*(adj.T > adj) - adj*(adj.T > adj)`
 *                   (utils.py:365) is max(adj, adj.T), i.e. MAX over the entries of adj and adj.T.
 * Non-finite duplicates stay in their own entry: under SUM a run holding inf sums to inf and a run
 * holding a NaN (or both infinities) to NaN; MAX is fmaxf, which ignores a NaN member — the entry
 * is NaN only if every member of its run is NaN.
 * Outputs: rowptr_out[n_rows+1] (int32 or int64), col_out / val_out with capacity nnz (sorted by
 * column inside every row), *nnz_out (DEVICE) = number of distinct entries.  All pointers DEVICE;
 * the caller guarantees 0 <= row < n_rows, 0 <= col < n_cols.  Deterministic, no atomics.
 */
#define GCN_REDUCE_SUM 0
#define GCN_REDUCE_MAX 1
size_t gcn_coo_to_csr_workspace_bytes(int64_t n_rows, int64_t n_cols, int64_t nnz);
int gcn_coo_to_csr_device(const int64_t *row, const int64_t *col, const float *val, int64_t nnz,
                          int64_t n_rows, int64_t n_cols, int reduce, void *rowptr_out,
                          int rowptr_is64, int32_t *col_out, float *val_out, int64_t *nnz_out,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * val <- D^-1 · val in place on the DEVICE: every stored entry is multiplied by the reciprocal of
 * the float32 sum of its row.  The reference's `normalize(mx)` (pygcn/utils.py:390-397), including
 * its `r_inv[isinf(r_inv)] = 0`: a row whose reciprocal is infinite — a sum of exactly 0, or a
 * subnormal sum below 2^-128 — becomes all zeros; so does a row whose sum overflows to +-inf (its
 * reciprocal is 0); a row that holds a NaN becomes NaN, its neighbours are untouched.
 */
int gcn_row_normalize_device(const void *rowptr, int rowptr_is64, float *val, int64_t n_rows,
                             void *stream);

/*
 * Y[M, 256] = X[M, 256] · W[256, 256] — the dense half of the layer, `torch.mm(input, weight)`
 * (pygcn/layers.py:33) and the grad_input GEMM of its backward, for the hidden width 256 of
 * configs C3/C4.  fp32 in / out / accumulate; operands are split into three bf16 parts on the
 * fly and multiplied with six bf16 MFMAs (fp32-level accuracy, see gcn_gemm.hip).  DEVICE
 * pointers; X rows 16-byte aligned; workspace >= gcn_gemm_xw256_workspace_bytes() (384 KiB).
 * W (here and in gcn_gemm_xw256_f32_h2 / _b3 / gcn_gemm_xw_bf16) needs no more than its element's
 * alignment and any ldw >= its width: a prep kernel reads it element by element into the workspace.
 * ldx, ldy (and ld_mask) >= the width, multiples of 16 bytes (GCN_E_ALIGN); nothing outside the M x
 * width window of Y is written (tests/test_gemm_exact_gpu.py).
 */
size_t gcn_gemm_xw256_workspace_bytes(void);
int gcn_gemm_xw256_f32(const float *X, int64_t ldx, const float *W, int64_t ldw, float *Y, int64_t ldy,
                       int64_t M, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same product by a cheaper decomposition: both operands are scaled by exact powers of two and
 * split into TWO fp16 parts, three fp16 MFMAs per product (half the matrix work of the 3 x bf16
 * form; error <= ~2^-21 relative per product, normwise ~1e-6 against an fp64 product).  fp16 has
 * little range, so the caller supplies x_absmax_bound: a DEVICE float holding any upper bound of
 * max|X| (the tighter, the more of fp16's 2^17 usable dynamic range is kept below the maximum;
 * elements further below it lose relative — not absolute — precision).  y_absmax: optional DEVICE
 * float, zeroed by the caller, receives max|Y| (atomic max) — the bound a following layer needs.
 * x_rows: optional DEVICE int32 list of M row indices — output row r is then the product of input
 * row x_rows[r] (the gradient GEMMs run on the rows that can be non-zero without a compacting
 * copy); NULL = rows 0 .. M-1.
 * epilogue: optional store-side options (struct gcn_gemm_epilogue below; NULL = plain product);
 * y_absmax reports the maximum of the values actually stored.
 * Workspace >= gcn_gemm_xw256_h2_workspace_bytes().  `torch.mm(input, weight)`, pygcn/layers.py:33.
 */
typedef struct gcn_gemm_epilogue {
    /* FORWARD epilogue, for a layer evaluated as (Â·X)·W + b — pygcn/layers.py:33-36 reassociated,
     * the GEMM being the layer's last stage (Fin <= Fout with a constant X: the product Â·X of the
     * forward pass is then also all the backward pass needs for grad_W, pygcn_amd/fused.py):
     *   y = acc + bias[col]; y = max(y, 0) if relu; y = keep ? y / (1 - p) : 0 if dropout_p > 0.
     * The keep bit is the SAME function of (seed, row, col) as in struct gcn_epilogue — Philox4x32-10 — so
     * a mask does not depend on which kernel stored the element; dropout requires relu. */
    const float *bias;        /* DEVICE fp32 [N] (N = 256 for the fp32 kernel), 16-byte aligned, or NULL */
    int32_t relu;
    float dropout_p;          /* in [0, 1); 0 disables dropout */
    uint64_t seed;
    const uint64_t *seed_dev; /* optional DEVICE seed read at execution time (hipGraph replays) */
    /* BACKWARD mask (excludes the forward epilogue): y = mask_src[input row, col] > 0 ? y *
     * mask_scale : 0 — the backward of a fused ReLU / dropout epilogue (out > 0 encodes ReLU and
     * keep, scale = 1 / (1 - p)) applied to the grad_input GEMM in its own store. */
    const float *mask_src;    /* DEVICE [*, N] in the GEMM's storage type — fp32 for gcn_gemm_xw256_f32_h2, bf16
                               * (passed through this pointer) for gcn_gemm_xw_bf16 — leading dimension ld_mask, or NULL;
                               * rows 16-byte aligned (GCN_E_ALIGN) */
    int64_t ld_mask;
    float mask_scale;
    /* optional DEVICE int32 list [M]: output row r reads mask row mask_rows[r]; NULL = the input
     * row (x_rows[r], or r).  For a COMPACT input whose rows belong to listed rows of a full mask. */
    const int32_t *mask_rows;
    /* added to the row index in the dropout counter (see struct gcn_epilogue; ABI 22) */
    int64_t drop_row_base;
    /* ABI 25, gcn_gemm_xw256_f32_b3 on CONTIGUOUS rows only (x_rows NULL; GCN_E_BADARG otherwise): the result of
     * the forward epilogue as ONE BIT per element — `out > 0`, which is all the backward of ReLU / dropout asks
     * of `out` — 32 bytes per row (DEVICE uint32 [M][8], 8-byte aligned) in the kernel's own lane order (an
     * opaque layout: only mask_bits of the same entry point reads it).  keep_bits_out: written next to Y by a
     * launch with relu and dropout_p in {0, 1/2}.  mask_bits: the backward mask read from such bits (row
     * mask_rows[r], or r) INSTEAD of mask_src — 32 bytes per row instead of 1 KiB; excludes the forward
     * epilogue like mask_src; mask_scale applies. */
    uint32_t *keep_bits_out;
    const uint32_t *mask_bits;
} gcn_gemm_epilogue;

size_t gcn_gemm_xw256_h2_workspace_bytes(void);
int gcn_gemm_xw256_f32_h2(const float *X, int64_t ldx, const int32_t *x_rows, const float *W,
                          int64_t ldw, float *Y, int64_t ldy, int64_t M, const float *x_absmax_bound,
                          float *y_absmax, const gcn_gemm_epilogue *epilogue, void *workspace,
                          size_t workspace_bytes, void *stream);

/*
 * The fp32-EQUIVALENT form of the same product (ABI 24) — what `torch.mm(input, self.weight)`
 * (pygcn/layers.py:33) computes in fp32: both operands split into THREE bf16 parts (a 24-bit
 * significand, fp32's own), six bf16 MFMAs per product (every term down to 2^-16 of the leading
 * one; the dropped ones are <= 2^-24), fp32 accumulation.  bf16 has fp32's exponent range: no
 * scaling and no bound.  The same options as gcn_gemm_xw256_f32_h2 — x_rows, y_absmax, the whole
 * struct gcn_gemm_epilogue.  Two kernels behind it, both deterministic: contiguous rows (x_rows NULL;
 * every epilogue but dropout at p != 1/2) run on 128-row tiles whose stores leave under the next
 * tile's MFMAs (K summed in chunks of 32); a row list runs round 3's pipeline (K in chunks of 16,
 * bit-identical to gcn_gemm_xw256_f32 for the plain product).  The two differ in fp32 summation
 * order only (<= 1e-6 of a row's largest entry).  Workspace >= gcn_gemm_xw256_b3_workspace_bytes().
 */
size_t gcn_gemm_xw256_b3_workspace_bytes(void);
int gcn_gemm_xw256_f32_b3(const float *X, int64_t ldx, const int32_t *x_rows, const float *W,
                          int64_t ldw, float *Y, int64_t ldy, int64_t M, float *y_absmax,
                          const gcn_gemm_epilogue *epilogue, void *workspace, size_t workspace_bytes,
                          void *stream);
/* Y = log_softmax(X · W + bias) row by row (additive to ABI 26) — `F.log_softmax(x, dim=1)` (pygcn/models.py:52
 * upstream) behind a last layer evaluated as (Â·h)·W + b: the contiguous-row kernel of gcn_gemm_xw256_f32_b3, whose
 * waves own whole rows, normalises a finished tile in its registers before it is stored (hardware exp2 / log2 as
 * in gcn_epilogue.log_softmax).  bias: DEVICE fp32 [256], 16-byte aligned, or NULL.  A row holding a NaN is NaN
 * throughout; no other row is.  ldx, ldy < 2^21; workspace >= gcn_gemm_xw256_b3_workspace_bytes(). */
int gcn_gemm_xw256_f32_b3_logsoftmax(const float *X, int64_t ldx, const float *W, int64_t ldw, const float *bias,
                                     float *Y, int64_t ldy, int64_t M, void *workspace, size_t workspace_bytes,
                                     void *stream);

/*
 * Y[M, N] = X[M, K] · W[K, N] for bf16 storage (config C5: 128 -> 128): bf16 in / out, fp32
 * accumulate, (K, N) one of (128,128), (128,256), (256,128).  HBM-bound by construction (W resident in LDS, X streamed
 * once, Y written once as 16-byte stores).  `torch.mm(input, weight)` (pygcn/layers.py:33) and
 * the grad_input GEMM of its backward at bf16.  DEVICE pointers; rows 16-byte aligned; workspace
 * >= gcn_gemm_bf16_workspace_bytes(K, N) (0 = unsupported shape).
 * epilogue: optional FORWARD epilogue, struct gcn_gemm_epilogue: bias fp32 [N], relu, dropout (
 * applied to the fp32 accumulators before the rounding to bf16, the order of the SpMM epilogue);
 * its backward-mask fields must be unset (GCN_E_BADARG).  NULL = plain product.
 */
size_t gcn_gemm_bf16_workspace_bytes(int64_t K, int64_t N);
int gcn_gemm_xw_bf16(const void *X, int64_t ldx, const void *W, int64_t ldw, void *Y, int64_t ldy,
                     int64_t M, int64_t K, int64_t N, const gcn_gemm_epilogue *epilogue,
                     void *workspace, size_t workspace_bytes, void *stream);

/*
 * out[256, 256] = Σ_{r < n_list} A[rows_a[r], :]ᵀ ⊗ G[rows_g[r], :]  — the weight gradient
 * `inputᵀ · grad_support` of `torch.mm(input, weight)` (pygcn/layers.py:33; autograd of the call
 * at pygcn/train.py:157) for 256-wide layers, fp32 in / out, over a LIST of rows: rows_a / rows_g
 * are DEVICE int32 index lists naming the rows on which the gradient can be non-zero (an identity
 * list for "all rows"), so the operands need not be compacted first; a list must be PADDED to a
 * multiple of 16 entries with valid indices (n_list counts the real ones).  Scaled two-part fp16
 * scheme as gcn_gemm_xw256_f32_h2 (a_absmax_bound / g_absmax_bound: DEVICE floats, upper bounds
 * of max|A|, max|G| over the listed rows); partial products of row slabs are added in slab order
 * (deterministic).  Rows of A and G 16-byte aligned (GCN_E_ALIGN).  Workspace >=
 * gcn_gemm_atg256_workspace_bytes(n_list).
 */
size_t gcn_gemm_atg256_workspace_bytes(int64_t n_list);
int gcn_gemm_atg256_f32(const float *A, int64_t lda, const int32_t *rows_a, const float *G, int64_t ldg,
                        const int32_t *rows_g, int64_t n_list, const float *a_absmax_bound,
                        const float *g_absmax_bound, float *out, int64_t ldo, void *workspace,
                        size_t workspace_bytes, void *stream);
/* The fp32-equivalent form (ABI 24): three bf16 parts per operand, six MFMAs per product, no
 * bounds (see gcn_gemm_xw256_f32_b3); same lists, workspace and determinism. */
int gcn_gemm_atg256_f32_b3(const float *A, int64_t lda, const int32_t *rows_a, const float *G, int64_t ldg,
                           const int32_t *rows_g, int64_t n_list, float *out, int64_t ldo, void *workspace,
                           size_t workspace_bytes, void *stream);
/* ... and (ABI 25) with the BIAS gradient of the same layer as a side result: colsum_g[256] (DEVICE
 * floats) = Σ_{r < n_list} G[rows_g[r], :] — `grad_output.sum(0)` of `output + self.bias`
 * (pygcn/layers.py:36) over the rows on which the gradient can be non-zero — summed from the rows the
 * kernel loads anyway (8 rows at a time, compensated running sums, workgroup partials added in
 * order in double precision: deterministic), instead of in a pass of its own over G. */
int gcn_gemm_atg256_f32_b3_colsum(const float *A, int64_t lda, const int32_t *rows_a, const float *G, int64_t ldg,
                                  const int32_t *rows_g, int64_t n_list, float *out, int64_t ldo, float *colsum_g,
                                  void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same weight gradient for bf16 STORAGE (config C5: 128 -> 128 layers): A [*, K] and G [*, N]
 * are bf16 (row-major, even leading dimensions, 4-byte aligned), accumulation and the [K, N] result
 * are fp32; no scaling and no bounds (bf16 has fp32's range).  (K, N) = (128, 128); the workspace
 * size is 0 for shapes the kernel does not carry (the caller then uses a library GEMM).  Row lists
 * as for gcn_gemm_atg256_f32 (padded to a multiple of 16 entries with valid indices).
 * Deterministic.  (ABI 22.)
 */
size_t gcn_gemm_atg_bf16_workspace_bytes(int64_t n_list, int64_t K, int64_t N);
int gcn_gemm_atg_bf16(const void *A, int64_t lda, const int32_t *rows_a, const void *G, int64_t ldg,
                      const int32_t *rows_g, int64_t n_list, int64_t K, int64_t N, float *out,
                      int64_t ldo, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Rows of a mostly-zero activation as BITMASK + NON-ZERO VALUES — the wire format of the multi-GPU
 * path's compressed hidden-layer halo exchange (pygcn_amd/sharded.py; the input of the second
 * GraphConvolution layer is relu + dropout output, pygcn/models.py:48,50: >= 75 % zeros in
 * training).  The reference has no multi-device code; SURVEY §8(e).  (ABI 22.)
 *   bit j of bits[r*(F/32) + w] is set iff element 32*w + j of row r is non-zero; vals holds the
 *   non-zero elements in row-major order, row r starting at offsets[r].
 * gcn_rows_pack_count : reads rows `rows[r]` (NULL = rows 0..m-1) of src [*, ld] (fp32 or bf16, F
 *   a multiple of 32, ld a multiple of 4, 16-byte aligned base); writes bits [m, F/32] and
 *   counts [m] (non-zeros per row).  The caller scans counts into offsets (int64, exclusive).
 * gcn_rows_pack_values: writes vals [offsets[m-1] + counts[m-1]] (element type of src).
 * gcn_rows_unpack     : dst [m, ldd] (every element written) from bits, offsets, vals.
 * gcn_bits_row_counts : counts [m] = set bits per row of bits [m, words] (the receiver's side:
 *   the wire carries bits and values only; it scans these counts into its own offsets).
 * -0.0 counts as zero (it compares equal to 0) and arrives as +0.0; NaN is non-zero.
 * Deterministic; DEVICE pointers; asynchronous on `stream`.
 */
int gcn_rows_pack_count(int dtype, const void *src, int64_t ld, const int64_t *rows, int64_t m, int64_t F,
                        uint32_t *bits, int32_t *counts, void *stream);
int gcn_rows_pack_values(int dtype, const void *src, int64_t ld, const int64_t *rows, int64_t m, int64_t F,
                         const int64_t *offsets, void *vals, void *stream);
int gcn_rows_unpack(int dtype, const uint32_t *bits, const int64_t *offsets, const void *vals, int64_t m,
                    int64_t F, void *dst, int64_t ldd, void *stream);
int gcn_bits_row_counts(const uint32_t *bits, int64_t m, int64_t words, int32_t *counts, void *stream);

/*
 * The FIXED-SLOT form of the same idea for the single-GPU layer-2 gather (additive to ABI 26): one 512-byte
 * slot per 256-wide fp32 row, so a gather needs no offsets and reads half the bytes of the dense row.
 *   slot r = words [128 r, 128 r + 128) of `slots`: four 128-byte sub-slots, one per column QUARTER in the lane
 *   order of gcn_gemm_xw256_f32_b3's keep bits — quarter q holds columns 16 cb + 4 q + j (cb 0..15, j 0..3) at bit
 *   4 cb + j.  Sub-slot q, 32 words: [0] [1] the 64-bit mask (bit set <=> the element's bit pattern is non-zero:
 *   -0.0 is kept, the slot reproduces the row bit for bit), [2] the number of set bits, [3 ..] the non-zero values
 *   in bit order.  A quarter with more than GCN_PACK512_CAPACITY set bits marks its row OVERFLOWED: its first 29
 *   values are stored and a reader takes the dense row instead.  Words past the count are left unwritten.
 * gcn_rows_pack512   : src [m, 256] fp32 (ld a multiple of 4, 16-byte aligned) -> slots [m][128] (16-byte aligned).
 *   One streaming pass: reads 1 KiB and writes at most 512 bytes per row.
 * gcn_spmm_csr_packed: C[n_rows, 256] = A · B with the rows of B gathered from `slots` (gcn_rows_pack512 of B);
 *   B itself is read for overflowed rows only.  The same products in the same order as gcn_spmm_csr on B: the
 *   result is bit-identical.  Workspace: gcn_spmm_workspace_bytes(plan, 256).  No epilogue.
 */
#define GCN_PACK512_CAPACITY 29
int gcn_rows_pack512(const float *src, int64_t ld, int64_t m, uint32_t *slots, void *stream);
int gcn_spmm_csr_packed(const gcn_csr_plan *plan, const uint32_t *slots, const float *B, int64_t ldb, float *C,
                        int64_t ldc, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The POOLED 384-byte form (additive to ABI 26): the same row with ONE pool of values, so the padding against a row
 * denser than the mean is paid once and not once per quarter — three whole 128-byte lines per gathered row.
 *   slot r = words [96 r, 96 r + 96) of `slots` (contiguous, 16-byte aligned; three whole lines per slot
 *   at a 128-byte aligned base, which is what the Python side allocates):
 *   [0 .. 7]   the masks: words 2q, 2q + 1 are quarter q's 64-bit mask, the quarters and bits of the 512-byte form
 *              (bit 4 cb + j of quarter q <=> column 16 cb + 4 q + j; set <=> the bit pattern is non-zero, so -0.0 is
 *              a stored value);
 *   [8]        the header, c_q = the number of set bits of quarter q: byte 0 = c0, byte 1 = c0 + c1, byte 2 = c0 + c1
 *              + c2 (where quarters 1, 2, 3 begin in the pool), byte 3 = min(c0 + c1 + c2 + c3, 255);
 *   [9 .. 95]  the values: quarter 0's in bit order, then quarter 1's, 2's and 3's.
 *   A row with more than GCN_PACK384_CAPACITY values is OVERFLOWED: masks and header are valid, its value words are
 *   undefined and a reader takes the dense row.  Words past 9 + total are undefined; no reader may depend on them.
 * gcn_rows_pack384      : src [m, 256] fp32 (ld a multiple of 4, 16-byte aligned) -> slots [m][96].  One streaming
 *   pass: reads 1 KiB and writes 384 bytes per row.
 * gcn_spmm_csr_packed384: gcn_spmm_csr_packed on the slots of gcn_rows_pack384 — the same products in the same
 *   order, bit-identical to gcn_spmm_csr on B.
 */
#define GCN_PACK384_CAPACITY 87
int gcn_rows_pack384(const float *src, int64_t ld, int64_t m, uint32_t *slots, void *stream);
int gcn_spmm_csr_packed384(const gcn_csr_plan *plan, const uint32_t *slots, const float *B, int64_t ldb, float *C,
                           int64_t ldc, void *workspace, size_t workspace_bytes, void *stream);

/*
 * ReLU + training-mode BatchNorm over the rows of a contiguous row-major [n_rows, F] activation —
 * the fork's live model normalises the output of its first two layers,
 *     x = self.apply_bn(F.relu(self.gc1(x, adj)))                 reference pygcn/models.py:49,53
 *     apply_bn: nn.BatchNorm1d(x.size()[1]).cuda()(x)             reference pygcn/models.py:41-45
 * (a fresh module per call: batch statistics, gamma = 1, beta = 0).  With x = relu ? relu(z) : z:
 *     mean[f] = mean_r x[r,f]    var[f] = mean_r (x[r,f] - mean[f])^2  (biased, as BatchNorm normalises)
 *     rstd = 1 / sqrt(var + eps) xhat = (x - mean) * rstd              y = xhat * gamma + beta
 *     backward, g = dL/dy:       sum_g = sum_r g  (= dbeta)            sum_gxhat = sum_r g * xhat  (= dgamma)
 *     dx = gamma * rstd * (g - sum_g / n - xhat * sum_gxhat / n)       dz = (relu && z <= 0) ? 0 : dx
 * as four sweeps: 3 activation-sized streams forward (stats: read z; apply: read z, write y) and 5
 * backward (sums: read g, z; apply: read g, z, write dz).  ReLU and its backward mask ride in the
 * loads; xhat is recomputed from z.  relu(NaN) = NaN and the mask passes dx where z is NaN, as torch.
 * `dtype` (fp32 / bf16) is the storage of z, y, g, dz: the forward arithmetic is fp32, results are
 * rounded once in the store; mean, var, rstd, gamma, beta, sum_g, sum_gxhat are DEVICE fp32 [F]; gamma
 * and beta may each be NULL (1 resp. 0).  The reductions carry their running sums in double and add
 * per-block partial rows in block order (no float atomics): deterministic, and the variance of a
 * column far from zero survives.
 * The backward pair works in double: over few rows dx cancels to eps * rstd^2 of its terms, and an
 * fp32 rounding of mean, rstd or a sum would come out multiplied by the inverse of that (3e-5 of
 * max|dz| at n_rows = 2).  gcn_bn_backward_sums therefore takes the fp32 `mean` of gcn_bn_stats only as
 * the centre of its sums, recovers the column's mean, var and rstd = 1 / sqrt(var + eps) to double
 * precision from z (which it reads anyway), and writes, besides sum_g and sum_gxhat, the DEVICE
 * double `coef`[4][F] = { mean, rstd, sum_g / n, rstd^2 * sum_r g (x - mean) / n } that
 * gcn_bn_backward_apply evaluates dx from (NULL: GCN_E_BADARG; 8-byte aligned).
 * Shape rule of gcn_relu_dropout_backward_colsum: F a multiple of the
 * 16-byte lane width v (4 fp32 / 8 bf16) with F/v dividing 256; that or n_rows < 2 is GCN_E_BADARG.
 * Tensors and workspace 16-byte aligned (GCN_E_ALIGN).  dz may alias g.
 * Scratch of the two reducing calls (0 for a shape outside the rule):
 *     gcn_bn_workspace_bytes = B * 4 * F * sizeof(double),  B = min(ceil(n_rows / 64), 2048) blocks,
 *     block b sweeping rows [b * R, min((b + 1) * R, n_rows)) with R = ceil(n_rows / B).
 * (ABI 26.)
 */
size_t gcn_bn_workspace_bytes(int64_t n_rows, int64_t F, int dtype);
int gcn_bn_stats(int dtype, const void *z, int64_t n_rows, int64_t F, int relu, float eps, float *mean,
                 float *var, float *rstd, void *workspace, size_t workspace_bytes, void *stream);
int gcn_bn_apply(int dtype, const void *z, void *y, int64_t n_rows, int64_t F, int relu, const float *mean,
                 const float *rstd, const float *gamma, const float *beta, void *stream);
int gcn_bn_backward_sums(int dtype, const void *g, const void *z, int64_t n_rows, int64_t F, int relu, float eps,
                         const float *mean, float *sum_g, float *sum_gxhat, double *coef, void *workspace,
                         size_t workspace_bytes, void *stream);
int gcn_bn_backward_apply(int dtype, const void *g, const void *z, void *dz, int64_t n_rows, int64_t F, int relu,
                          const float *gamma, const double *coef, void *stream);

/*
 * The same four sweeps over `batch` COLUMN WINDOWS of a contiguous row-major [n_rows, batch * F] matrix:
 * window j is the columns [j * F, (j + 1) * F), read with the row pitch batch * F.  This is the layout in
 * which GraphConvolution holds k samples over one graph side by side, so that per-sample BatchNorm — the
 * fork runs its model once per sample in a Python loop, "cannot batch yet", reference
 * pygcn/models.py:343-349 — is per-column BatchNorm of ONE matrix, in one launch per sweep.
 * F obeys the shape rule above (the WINDOW width; batch * F is free), 1 <= batch <= 65535 (else
 * GCN_E_BADARG).  The per-column vectors mean, var, rstd, sum_g, sum_gxhat, gamma, beta have batch * F
 * entries (window after window; gamma, beta may be NULL), coef is [4][batch * F] double.
 * A window's results are BITWISE those of the 2-D entry point on a contiguous [n_rows, F] copy of the
 * window, whatever `batch` is: same slabs, same lanes, same summation orders (the 2-D entry points are
 * the batch = 1 launch of the same kernels).  Errors, alignment, NaN / inf and aliasing as above.
 *     gcn_bn_batched_workspace_bytes = batch * gcn_bn_workspace_bytes(n_rows, F, dtype)
 * (window j's partial rows at byte j * gcn_bn_workspace_bytes); 0 outside the rule.
 * (ABI 26, additive.)
 */
size_t gcn_bn_batched_workspace_bytes(int64_t n_rows, int64_t F, int64_t batch, int dtype);
int gcn_bn_stats_batched(int dtype, const void *z, int64_t n_rows, int64_t F, int64_t batch, int relu, float eps,
                         float *mean, float *var, float *rstd, void *workspace, size_t workspace_bytes,
                         void *stream);
int gcn_bn_apply_batched(int dtype, const void *z, void *y, int64_t n_rows, int64_t F, int64_t batch, int relu,
                         const float *mean, const float *rstd, const float *gamma, const float *beta, void *stream);
int gcn_bn_backward_sums_batched(int dtype, const void *g, const void *z, int64_t n_rows, int64_t F, int64_t batch,
                                 int relu, float eps, const float *mean, float *sum_g, float *sum_gxhat,
                                 double *coef, void *workspace, size_t workspace_bytes, void *stream);
int gcn_bn_backward_apply_batched(int dtype, const void *g, const void *z, void *dz, int64_t n_rows, int64_t F,
                                  int64_t batch, int relu, const float *gamma, const double *coef, void *stream);

/*
 * Masked column sums over the same layout — the reduction of the fork's PoolLayer (reference
 * pygcn/models.py:267-286: every sample's [N, C] output is multiplied by a 0/1 vertex mask, summed over
 * the vertices and divided by a vertex count).  h is a contiguous [n_rows, batch * C] matrix (fp32 / bf16),
 * mask a contiguous fp32 [batch, n_rows] (sample after sample, as the fork holds it):
 *     gcn_masked_colsum      sums[j * C + c] = sum_r mask[j, r] * h[r, j * C + c]        one read sweep
 *     gcn_masked_broadcast   dh[r, j * C + c] = mask[j, r] * coef[j * C + c]             one write sweep
 * `sums` is DEVICE double [batch * C] (8-byte aligned): products and sums are carried in double per
 * thread, per block and in the finish kernel, added in a fixed order — no float atomics, bitwise
 * reproducible; the division by the count is the caller's.  The mask MULTIPLIES (0 * NaN = NaN, as in
 * the fork).  `coef` is DEVICE fp32 [batch * C]; the product is fp32, rounded once in the store of dh.
 * C obeys the shape rule above, n_rows >= 1, 1 <= batch <= 65535 (else GCN_E_BADARG); h, dh and the
 * workspace 16-byte aligned (GCN_E_ALIGN).
 *     gcn_pool_workspace_bytes = batch * B * C * sizeof(double),  B = min(ceil(n_rows / 64), 2048);
 * 0 outside the rule.
 * (ABI 26, additive.)
 */
size_t gcn_pool_workspace_bytes(int64_t n_rows, int64_t C, int64_t batch, int dtype);
int gcn_masked_colsum(int dtype, const void *h, const float *mask, int64_t n_rows, int64_t C, int64_t batch,
                      double *sums, void *workspace, size_t workspace_bytes, void *stream);
int gcn_masked_broadcast(int dtype, const float *mask, const float *coef, void *dh, int64_t n_rows, int64_t C,
                         int64_t batch, void *stream);

/*
 * Vertex attention over the same layout — the head of the fork's SoftGenerator (reference
 * pygcn/models.py:324-329: attn = softmax over the vertices of torch.mul(key, x).sum(dim=1)).  h is a
 * contiguous [n_rows, batch * C] matrix (fp32 / bf16), key DEVICE fp32 [batch * C]; every per-row vector
 * (scores, attn, ds) is fp32 [batch, n_rows], one window's rows consecutive, as the pool's mask.  Per window j:
 *     s_r = sum_c key[j, c] * h[r, j * C + c]      M = max_r s_r      Z = sum_r exp(s_r - M)
 *     attn_r = exp(s_r - M) / Z
 *     backward, ds_r = attn_r * (g_r - sum_r g_r attn_r) formed by the caller ([batch, n_rows] work):
 *     dh[r, j * C + c] = ds_r * key[j, c]          dkey[j, c] = sum_r ds_r * h[r, j * C + c]
 *   gcn_attn_scores     one read sweep of h: the dot is carried in double, rounded ONCE and stored as
 *                       scores[j, r]; the same launch reduces (M, Z) in double over each block's slab FROM
 *                       THE ROUNDED SCORE (every later pass sees the same number), one pair per block and
 *                       window, and a finish launch merges the pairs in a fixed order into
 *                       `stats`, DEVICE double [batch, 2] = (M_j, Z_j), 8-byte aligned.
 *   gcn_attn_normalize  attn[j, r] = (float)(exp((double)scores[j, r] - M_j) / Z_j): a pass over
 *                       [batch, n_rows] floats; attn may alias scores.
 *   gcn_attn_backward   one sweep: reads h and ds, writes dh (fp32 product, rounded once in the store) and
 *                       accumulates dkey in double exactly as gcn_masked_colsum accumulates its sums; a finish
 *                       launch writes `dkey`, DEVICE double [batch * C], 8-byte aligned.  dh may be NULL: the
 *                       store is skipped and the call is one read of h.
 * No float atomics, every sum in a fixed order: bitwise reproducible, and window j of a batched call is,
 * bit for bit, the batch = 1 call on a contiguous copy of the window.  A NaN in a window's h makes that
 * window's attn all NaN (torch's softmax) and leaves the other windows' bits alone.
 * C obeys the shape rule above, n_rows >= 1, 1 <= batch <= 65535 (else GCN_E_BADARG); h, dh and the
 * workspace 16-byte aligned (GCN_E_ALIGN).  Scratch of gcn_attn_scores and gcn_attn_backward:
 *     gcn_attn_workspace_bytes = batch * B * max(C, 2) * sizeof(double),  B = min(ceil(n_rows / 64), 2048);
 * 0 outside the rule.
 * (ABI 26, additive.)
 */
size_t gcn_attn_workspace_bytes(int64_t n_rows, int64_t C, int64_t batch, int dtype);
int gcn_attn_scores(int dtype, const void *h, const float *key, int64_t n_rows, int64_t C, int64_t batch,
                    float *scores, double *stats, void *workspace, size_t workspace_bytes, void *stream);
int gcn_attn_normalize(const float *scores, const double *stats, float *attn, int64_t n_rows, int64_t batch,
                       void *stream);
int gcn_attn_backward(int dtype, const void *h, const float *ds, const float *key, void *dh, double *dkey,
                      int64_t n_rows, int64_t C, int64_t batch, void *workspace, size_t workspace_bytes,
                      void *stream);

/*
 * Vertex selection over the same per-vertex layout — how every policy generator of the fork ends: the top-NN
 * flag of Generator / Hierarchical_Generator (reference pygcn/models.py:373-377, :398-406: argsort, compare
 * with the score at index NN) and SoftGenerator's draw of NN vertices without replacement (reference
 * pygcn/rl-policy-generator.py:324-336: torch.multinomial + .tolist()).  Every per-vertex vector (keys, s,
 * flag, p) is fp32 [batch, n_rows], contiguous, one window's rows consecutive; 1 <= n_rows < 2^31,
 * 1 <= batch <= 65535 (else GCN_E_BADARG).  Nothing is read back by the host.
 *
 * ORDER.  All selection uses one total order on fp32: -0 is +0; every NaN (any sign, any payload) is greater
 * than +inf, which is where torch.argsort(descending=True) places it; otherwise the numeric order.  (The
 * order-preserving uint32: all bits of a negative flipped, the sign bit of a non-negative set, NaN 0xFFFFFFFF.)
 *
 *   gcn_select_kth      thr[j] = the kth-largest key of window j in that order (kth 1-based, 1 <= kth <= n_rows;
 *                       a NaN comes back as 0x7FC00000 and a zero as +0) and count_gt[j] = the number of keys
 *                       strictly greater; DEVICE fp32 [batch] and int32 [batch].  A radix select over 11 / 11 /
 *                       10 bits from the top: seven launches — one that zeroes the scratch, then per digit a
 *                       read sweep whose blocks count the keys that match the digits found so far in LDS bins
 *                       (integer atomics) and add them to the window's bins (integer atomics), and a one-block
 *                       step that picks the digit and carries prefix, remaining rank and count in the scratch.
 *   gcn_select_indices  idx[j, 0 .. m) (DEVICE int64 [batch, m], 8-byte aligned, 1 <= m <= n_rows) = the
 *                       vertices whose key is greater than thr[j], plus the lowest-index vertices whose key
 *                       equals it, until there are m; ascending vertex order.  thr and count_gt are
 *                       gcn_select_kth's results for kth = m (other values write only inside idx and may
 *                       leave slots unwritten).  Three launches: count per block, scan, write.
 *   gcn_topk_flag       flag[j, r] = s[j, r] > thr[j] ? s[j, r] * (1.0f / s[j, r]) : 0 with the ordinary float
 *                       comparison (a NaN score or threshold selects nothing); quotient and product are each
 *                       rounded to fp32 once, IEEE: the bits of `s * torch.reciprocal(s)`, 0 * inf = NaN
 *                       included.  An unselected vertex gets +0 whatever its score (the fork's `s * 0` leaves
 *                       NaN for a NaN or infinite score).  flag may alias s.
 *   gcn_race_keys       the keys of an exponential race: the m largest of p_r / E_r, E_r i.i.d. Exp(1), are m
 *                       draws without replacement with probabilities proportional to p.  For vertex r of window j
 *                           w   = Philox4x32-10(counter = (q_lo, q_hi, j, 1), key = (seed_lo, seed_hi)),  q = r >> 2
 *                           u   = (w[r & 3] + 0.5) * 2^-32          in double (exact)
 *                           E   = -log(u)                           in double; 1.16e-10 <= E <= 22.9
 *                           key = (float)((double)p / E)            rounded once
 *                       (the dropout stream has counter word 3 = 0: one seed never gives both the same bits).
 *                       p = 0 gives key +0: such a vertex is taken after every positive one, lowest index first.
 *                       A negative or non-finite p is the CALLER'S ERROR and is not detected (torch.multinomial
 *                       raises, which needs a host read).  keys may alias p.
 *   gcn_race_keys_dev   gcn_race_keys with the seed read from *seed_dev (DEVICE uint64, 8-byte aligned) when the
 *                       kernel RUNS, as gcn_epilogue.seed_dev is: a launch captured into a hipGraph draws anew on
 *                       every replay if the graph also advances *seed_dev.  The bits of gcn_race_keys(seed = *seed_dev).
 *                       (Added without moving the ABI number.)
 * Integer atomics and fixed-order scans only: two runs give the same bytes, and window j of a batched call is,
 * bit for bit, the batch = 1 call on a contiguous copy of the window.  Tensors 4-byte aligned (GCN_E_ALIGN).
 * Scratch of gcn_select_kth and gcn_select_indices, which the caller need not initialise:
 *     gcn_select_workspace_bytes = batch * (3 * 2048 + 8 + 2 * B) * sizeof(int32_t),  B = min(ceil(n_rows / 1024), 1024);
 * block b of a window sweeps rows [b * R, min((b + 1) * R, n_rows)), R = ceil(n_rows / B), 256 rows per
 * iteration.  0 outside the rule; a short or NULL workspace is GCN_E_WORKSPACE.
 * (ABI 26, additive.)
 */
size_t gcn_select_workspace_bytes(int64_t n_rows, int64_t batch);
int gcn_select_kth(const float *keys, int64_t n_rows, int64_t batch, int64_t kth, float *thr, int32_t *count_gt,
                   void *workspace, size_t workspace_bytes, void *stream);
int gcn_select_indices(const float *keys, int64_t n_rows, int64_t batch, int64_t m, const float *thr,
                       const int32_t *count_gt, int64_t *idx, void *workspace, size_t workspace_bytes, void *stream);
int gcn_topk_flag(const float *s, int64_t n_rows, int64_t batch, const float *thr, float *flag, void *stream);
int gcn_race_keys(const float *p, int64_t n_rows, int64_t batch, uint64_t seed, float *keys, void *stream);
int gcn_race_keys_dev(const float *p, int64_t n_rows, int64_t batch, const uint64_t *seed_dev, float *keys,
                      void *stream);

/*
 * The input side of the fork's evaluator GCN_OVER_MLP (reference pygcn/models.py:333-355, PoolLayer :267-286) as one
 * read sweep of x and one write sweep of dx.  x is a contiguous fp32 [batch, n_rows, F] tensor, sample after
 * sample, as the fork holds it (reference pygcn/gnn-over-mlp.py:219-237, F = 9 or 17): the columns [0, d) feed the
 * GCN (d = its dim_touched), the e = F - 1 - d columns [d, F-1) are pooled as they are, and the last column is the
 * 0/1 vertex flag the pool multiplies by and counts.  m(j, n) is flag[j, n] when `flag` (contiguous fp32
 * [batch, n_rows]) is not NULL, and x[j, n, F-1] otherwise.
 *   gcn_eval_ingest           one read of x (and flag); every output pointer may be NULL, that output is skipped:
 *       wide[n, j * d + c]   = x[j, n, c], c < d          fp32 [n_rows, batch * d], the layout the batched layers
 *                                                         keep (k samples side by side); a pure copy
 *       mask[j, n]           = m(j, n)                    fp32 [batch, n_rows], the layout gcn_masked_colsum reads
 *       esum[j * e + c - d]  = sum_n m(j, n) * x[j, n, c], d <= c < F-1     DEVICE double [batch * e], 8-byte
 *                              aligned: products and sums are carried in double per thread, per block and in a
 *                              finish launch, added in a fixed order — no float atomics, bitwise reproducible.
 *                              The mask MULTIPLIES (0 * NaN = NaN, as in the fork).
 *       nonzero[j]           = #{n : m(j, n) != 0}        DEVICE int64 [batch], 8-byte aligned; a NaN counts, as
 *                              torch.nonzero counts it; integer adds only.
 *   gcn_eval_ingest_backward  one sweep: reads x (and flag), d_wide [n_rows, batch * d], d_mask [batch, n_rows] and
 *                             d_esum fp32 [batch * e] — each of the three gradients may be NULL, which means zero —
 *                             and writes dx [batch, n_rows, F]:
 *       dx[j, n, c < d]        = d_wide[n, j * d + c]
 *       dx[j, n, d <= c < F-1] = m(j, n) * d_esum[j * e + c - d]          one fp32 product, rounded once
 *       dm(j, n)               = d_mask[j, n] + sum_c x[j, n, c] * d_esum[j * e + c - d]    in double, rounded once
 *                             Without `flag`, dm goes to dx[j, n, F-1].  With `flag`, dm goes to dflag[j, n] (fp32
 *                             [batch, n_rows]; may be NULL) and dx[j, n, F-1] = 0.  dx may be NULL when flag and
 *                             dflag are given: the sweep then reads only the columns >= d of x and writes
 *                             batch * n_rows floats.  dflag without flag, or neither dx nor dflag, is GCN_E_BADARG.
 * Both sweeps stage tiles of 64 consecutive vertices x as many samples as fit 32 KiB through LDS (a block may take a
 * sub-range of the samples, on gridDim.y), so that every global access is a run of consecutive dwords: of a sample's
 * flat array on the x / dx side, of a row of wide / d_wide on the other, of one sample's mask.
 * SHAPE RULE: n_rows >= 1, 2 <= F <= 64, 0 <= d <= F - 1, 1 <= batch <= 65535 (else GCN_E_BADARG); x NULL is
 * GCN_E_BADARG.  Every fp32 tensor 4-byte aligned, esum and nonzero 8-byte, the workspace 16-byte (GCN_E_ALIGN).
 * Scratch of gcn_eval_ingest, needed when esum or nonzero is asked for (short or NULL: GCN_E_WORKSPACE):
 *     gcn_eval_workspace_bytes = B * batch * (F - d) * sizeof(double),  B = min(ceil(n_rows / 64), 2048)
 * — per block batch * e partial sums and batch partial counts; block b sweeps the rows [b * R, min((b + 1) * R,
 * n_rows)), R = 64 * ceil(n_rows / (64 * B)), in tiles of 64.  0 outside the rule.
 * (ABI 26, additive.)
 */
size_t gcn_eval_workspace_bytes(int64_t n_rows, int64_t F, int64_t d, int64_t batch);
int gcn_eval_ingest(const float *x, const float *flag, int64_t n_rows, int64_t F, int64_t d, int64_t batch,
                    float *wide, float *mask, double *esum, int64_t *nonzero, void *workspace,
                    size_t workspace_bytes, void *stream);
int gcn_eval_ingest_backward(const float *x, const float *flag, const float *d_wide, const float *d_mask,
                             const float *d_esum, int64_t n_rows, int64_t F, int64_t d, int64_t batch, float *dx,
                             float *dflag, void *stream);

/*
 * The per-vertex score head of the fork's Generator and Hierarchical_Generator (reference pygcn/models.py:368-370,
 * :391-393, the two MLPs :195-241) as fused sweeps that recompute the hidden activations instead of storing them:
 *     score[n] = linear3( bn(relu( linear2( bn(relu( linear1( cat(h[n, :], x[n, d : d + T]) ))) )) ))
 * h fp32 [n_rows, C] contiguous; x fp32 with row pitch ldx floats, of which only the columns [d, d + T) are read
 * (the concatenation never exists; x may be NULL when T = 0); W1 [H1, C + T], W2 [H2, H1], W3 [1, H2] in the
 * nn.Linear layout; the biases b1 [H1], b2 [H2], b3 [1] may each be NULL (zero).  batch_norm != 0: after each ReLU
 * the fork's FRESH BatchNorm1d — batch statistics over all n_rows, biased variance, eps 1e-5, gamma 1, beta 0;
 * batch_norm = 0: the plain MLPLayers.
 *   forward   scores fp32 [n_rows].  stats fp32 [4 * 64] (mean1, rstd1, mean2, rstd2 at pitch 64; written with
 *             batch_norm, else untouched and may be NULL) — what the backward call reads.  mask1, mask2: int64
 *             [n_rows], both or neither (NULL): bit j set when column j of that hidden layer counted as > 0.
 *             3 sweeps with batch_norm (statistics of layer 1, of layer 2, the score), 1 without.
 *   backward  dscores fp32 [n_rows] -> dh fp32 [n_rows, C] and the parameter gradients in the parameters' layouts;
 *             dh and each of the six may be NULL (skipped).  3 sweeps with batch_norm, 1 without.
 * Column sums are carried in double, the weight-gradient outer products in fp32 per wave over its slab of rows; one
 * partial row per block, added in a fixed order in double by a finish launch: no float atomics, bitwise
 * reproducible.  Nothing allocates or synchronises; capturable.
 * SHAPE RULE: n_rows >= 64, 1 <= C <= 64, 0 <= T <= 32, 1 <= H1, H2 <= 64, ldx >= d + T, d >= 0 (else
 * GCN_E_BADARG, also for a NULL h, W, scores / dscores, or stats with batch_norm).  fp32 tensors 4-byte
 * aligned, masks 8-byte, the workspace 16-byte (GCN_E_ALIGN).  Scratch of both calls (short or NULL:
 * GCN_E_WORKSPACE), with HP = max(H1, H2) rounded up to 16 / 32 / 64, K = C + T, B = min(ceil(n_rows / 64), 2048):
 *     B * (1 + 3 HP) doubles + B * (K + HP) * HP floats + (1 + 3 HP + (K + HP) * HP) doubles + 256 floats,
 * each part rounded up to 16 bytes — independent of n_rows above 2048 tiles; 0 outside the rule.  Block b sweeps
 * the rows [b * R, min((b + 1) * R, n_rows)), R = 64 * ceil(n_rows / (64 * B)), in tiles of 64, a wave per tile.
 * (ABI 26, additive.)
 */
size_t gcn_vmlp_workspace_bytes(int64_t n_rows, int64_t C, int64_t T, int64_t H1, int64_t H2);
int gcn_vmlp_forward(const float *h, const float *x, int64_t ldx, int64_t d, int64_t n_rows, int64_t C, int64_t T,
                     const float *W1, const float *b1, int64_t H1, const float *W2, const float *b2, int64_t H2,
                     const float *W3, const float *b3, int batch_norm, float *stats, float *scores, int64_t *mask1,
                     int64_t *mask2, void *workspace, size_t workspace_bytes, void *stream);
int gcn_vmlp_backward(const float *h, const float *x, int64_t ldx, int64_t d, int64_t n_rows, int64_t C, int64_t T,
                      const float *W1, const float *b1, int64_t H1, const float *W2, const float *b2, int64_t H2,
                      const float *W3, const float *b3, int batch_norm, const float *stats, const float *dscores,
                      float *dh, float *gW1, float *gb1, float *gW2, float *gb2, float *gW3, float *gb3,
                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * What a forward pass RESTRICTED to the receptive field of the loss rows needs beside the products (the model
 * evaluated on the rows R2 that the loss rows read, pygcn_amd/fused.py): compact tensors whose row r stands for
 * row rows[r] of the full-height tensor, and the matching row blocks of the adjacency.
 *
 *   gcn_dropout_rows   IN PLACE on h [m, F] (dtype fp32 / bf16, row pitch ld >= F elements):
 *                          h[r, f] = keep(seed, rows[r] + drop_row_base, f) ? h[r, f] * s : 0
 *                      with keep and s EXACTLY the dropout rule of struct gcn_epilogue above — both forms, eight
 *                      16-bit fields for T != 32768 and 128 one-bit fields at p = 1/2; counter word 3 = 0, row_lo /
 *                      row_hi the two words of the 64-bit row, s = 65536 / (65536 - T) — so at equal seed a compact
 *                      pass draws the mask the full-height launches draw.  rows: DEVICE int64 [m], any order,
 *                      repeats allowed, any 64-bit value (it only enters the counter; no memory is indexed by it);
 *                      NULL means rows[r] = r.  seed_dev: optional DEVICE seed, read when the kernel runs (as in
 *                      struct gcn_epilogue); NULL uses `seed`.  A dropped element becomes +0; a kept bf16 element is
 *                      multiplied in fp32 and rounded once (nearest-even).  Any F >= 1 and any pitch: runs of four
 *                      elements travel as one vector access where h is aligned to four elements and ld a multiple of
 *                      four, else element by element.  Nothing outside the m x F window is written.  One Philox call
 *                      serves all the columns it covers (8, or 128 at p = 1/2); no atomics, nothing read by the
 *                      host.  dropout_p = 0 or m = 0 launch nothing.  dropout_p outside [0, 1), m < 0, F < 1 or
 *                      ld < F is GCN_E_BADARG.
 *   gcn_csr_take_rows  rows of a CSR matrix as a CSR matrix: output row r receives the stored entries of input row
 *                      rows[r], in their stored order.  rows: DEVICE int64 [m], each in [0, n_rows) — the CALLER'S
 *                      duty, it is not checked — in any order, repeats allowed.  rowptr_out [m + 1] (int32, or
 *                      int64 with out_is64) is SUPPLIED by the caller: the exclusive scan of the selected rows'
 *                      lengths; col_out / val_out have rowptr_out[m] entries (the count stays on the device: a
 *                      fixed grid strides over it).  col_map (DEVICE int32 [n_cols], or NULL = columns unchanged)
 *                      renumbers the columns c -> col_map[c]; an entry with col_map[c] < 0 is written as column 0
 *                      with value 0 and adds 1 to the DEVICE int32 *n_unmapped (zeroed by the caller; may be NULL) —
 *                      a guard for a map that is meant to cover every column of the selected rows: the result then
 *                      stays a valid matrix with a zero entry, and the caller reads the count once.  One thread per
 *                      output entry, its row found by binary search in rowptr_out: consecutive threads store
 *                      consecutive entries; no float atomics, two runs give the same bytes.  An output slot that
 *                      rowptr_out places past the end of its input row is written as (0, 0).  m < 0 is
 *                      GCN_E_BADARG; m = 0 launches nothing.
 * (ABI 26, additive.)
 */
int gcn_dropout_rows(int dtype, void *h, int64_t ld, const int64_t *rows, int64_t m, int64_t F, float dropout_p,
                     uint64_t seed, const uint64_t *seed_dev, int64_t drop_row_base, void *stream);
int gcn_csr_take_rows(const void *rowptr, int rowptr_is64, const int32_t *col, const float *val, const int64_t *rows,
                      int64_t m, const int32_t *col_map, const void *rowptr_out, int out_is64, int32_t *col_out,
                      float *val_out, int32_t *n_unmapped, void *stream);

/*
 * BN(relu(z)) · W as one node for 32-wide layers: the fork's apply_bn(F.relu(gc(x, adj))) (reference
 * pygcn/models.py:49,53) folded into the NEXT layer's X·W (pygcn/layers.py:33), so that the normalised activation
 * is never written (pygcn_amd/csrc/gcn_normlin.hip).  z, s, ds, dz are contiguous fp32 [n_rows, batch * 32]: batch
 * samples side by side, the layout of the gcn_bn_*_batched entry points; weight is fp32 [Fin, Fout] row-major
 * (GraphConvolution's).  With x = relu ? relu(z) : z and xhat = (x - mean) * rstd per column of a window, mean and
 * rstd fp32 [batch * 32] as gcn_bn_stats_batched returns them:
 *   gcn_bn_linear_forward         s[:, window j] = xhat[:, window j] · weight.  xhat is formed in fp32 exactly as
 *                                 gcn_bn_apply_batched forms it (gamma, beta NULL) and the product is an fp32 fmaf
 *                                 chain (v_mfma_f32_32x32x2_f32).
 *   gcn_bn_linear_backward_sums   grad_w [Fin, Fout] fp32 = sum over windows and rows of xhat^T · ds, and the DEVICE
 *                                 double coef [4, batch * 32] in the layout gcn_bn_backward_sums_batched writes
 *                                 (mean, rstd, sum dy / n, rstd^2 * sum dy (x - mean) / n; dy = ds · weight^T, which
 *                                 is never stored).  fp32 sums run over one wavefront's slab of rows at most; the 4
 *                                 wavefronts of a block are added in wave order in double, one partial row per
 *                                 (window, block); a finish launch adds the partial rows of a window in a fixed
 *                                 order in double, a second one the windows in window order.  No float atomics,
 *                                 bitwise reproducible.
 *   gcn_bn_linear_backward_apply  dz = [z > 0] * rstd * (dy - sum dy / n - xhat * sum (dy xhat) / n), evaluated in
 *                                 double from coef as gcn_bn_backward_apply_batched does; dz must not alias ds.
 * A window's s, coef and dz are bitwise those of the batch = 1 call on a contiguous copy of the window.
 * SHAPE RULE: 2 <= n_rows <= 2^40, Fin = Fout = 32, 1 <= batch <= 65535 (else GCN_E_BADARG, as a NULL pointer);
 * z, s, ds, dz, weight and the workspace 16-byte aligned, coef 8-byte (GCN_E_ALIGN).
 * Scratch of gcn_bn_linear_backward_sums (short or NULL: GCN_E_WORKSPACE):
 *     gcn_bn_linear_workspace_bytes = batch * (B + 1) * 1152 * sizeof(double),
 *     T = ceil(n_rows / (128 * 512)),  R = 128 * T,  B = ceil(n_rows / R)
 * — every sweep runs B blocks of 4 wavefronts per window; block b owns the rows [b * R, min((b + 1) * R, n_rows)) and
 * its wavefront w the rows [b * R + 32 * T * w, b * R + 32 * T * (w + 1)) of them, walked in T tiles of 32 rows (the
 * last one partial where the slab ends).  0 outside the rule.
 * (ABI 26, additive.)
 */
size_t gcn_bn_linear_workspace_bytes(int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch);
int gcn_bn_linear_forward(const float *z, const float *weight, const float *mean, const float *rstd, float *s,
                          int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch, int relu, void *stream);
int gcn_bn_linear_backward_sums(const float *ds, const float *z, const float *weight, const float *mean,
                                const float *rstd, int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch,
                                int relu, float eps, float *grad_w, double *coef, void *workspace,
                                size_t workspace_bytes, void *stream);
int gcn_bn_linear_backward_apply(const float *ds, const float *z, const float *weight, const double *coef, float *dz,
                                 int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch, int relu, void *stream);

/*
 * Symmetric adjacencies (pygcn_amd/csrc/gcn_symmetric.hip).  All pointers DEVICE; nothing is read by the host.
 *   gcn_sym_normalize_device  val <- D^-1/2 · val · D^-1/2 in place for a SQUARE CSR matrix (Kipf & Welling's
 *                      normalisation; gcn_row_normalize_device is the reference's D^-1 form): entry e = (i, j)
 *                      becomes (float)((double)val[e] / sqrt(d_i * d_j)), d = the row sums in DOUBLE, summed in a
 *                      fixed order (lane-strided partials of one wavefront per row, then a shuffle tree), so two runs
 *                      give the same bytes.  The product d_i * d_j is formed first and commutes, so (i, j) and (j, i)
 *                      evaluate the same expression on the same operands: a matrix with bitwise symmetric weights
 *                      comes out bitwise symmetric.  d_i * d_j == 0 gives 0 (`d_inv_sqrt[isinf] = 0`); a NaN in a row
 *                      makes the entries of that row and of that column NaN and nothing else; a negative product
 *                      gives NaN, as numpy's power does.  Two launches: the degrees into the workspace (double
 *                      [n_rows], gcn_sym_normalize_workspace_bytes), then the scaling.  rowptr int32 or int64.
 *   gcn_csr_mirror_device     for every stored entry e = (i, j) of a square CSR matrix, mirror[e] = the storage
 *                      position of (j, i) — the lower bound of i among the columns of row j, if that position holds
 *                      i — or -1.  counts: DEVICE int64 [4], zeroed here and filled by the kernels:
 *                        [0] entries with no mirror;  [1] entries with mirror[mirror[e]] != e (duplicates);
 *                        [2] entries whose column is not above that of the entry before them in their row;
 *                        [3] entries whose value differs bitwise from their mirror's.
 *                      [0] = [1] = [2] = 0 says: sorted, unique, pattern-symmetric — CSR(A^T) then has A's rowptr and
 *                      col, and val_t[e] = val[mirror[e]].  One thread per entry (its row by binary search in rowptr),
 *                      so a row of any length costs no more than its entries; every probe stays inside
 *                      [rowptr[j], rowptr[j + 1]).  int32 rowptr only (nnz < 2^31): mirror holds 32-bit positions.
 *   gcn_gather_f32     out[e] = src[index[e]] for e < n; an index outside [0, src_len) gives 0.
 * (ABI 26, additive.)
 */
size_t gcn_sym_normalize_workspace_bytes(int64_t n_rows);
int gcn_sym_normalize_device(const void *rowptr, int rowptr_is64, const int32_t *col, float *val, int64_t n_rows,
                             void *workspace, size_t workspace_bytes, void *stream);
int gcn_csr_mirror_device(const int32_t *rowptr, const int32_t *col, const float *val, int64_t n_rows, int64_t nnz,
                          int32_t *mirror, int64_t *counts, void *stream);
int gcn_gather_f32(const float *src, const int32_t *index, int64_t n, int64_t src_len, float *out, void *stream);

/*
 * The dense half of an AGGREGATE-FIRST input layer, (A·X)·W + b, for narrow inputs (pygcn_amd/csrc/gcn_agglin.hip):
 * the fork's models feed 4, 8 or 16 columns into a 32-wide GCN (reference pygcn/gnn-over-mlp.py:221-237,
 * policy-generator.py:330-350) and layer 1's input needs no gradient, so with z = A·X formed by gcn_spmm_csr on
 * Fin-wide rows, the layer and its parameter gradients are two dense sweeps.  z is contiguous fp32
 * [n_rows, batch * Fin], y and g contiguous fp32 [n_rows, batch * Fout]: batch samples side by side, sample j in the
 * columns [j * F, (j + 1) * F) — so row r, sample j is "unit" u = r * batch + j, Fin contiguous floats of z and
 * Fout contiguous floats of y.  weight is fp32 [Fin, Fout] row-major (GraphConvolution's), bias fp32 [Fout] or NULL.
 *   gcn_agg_linear_forward    y[r, j * Fout + c] = act(sum_i z[r, j * Fin + i] * weight[i, c] + bias[c]).  THE ORDER,
 *                             per element, in fp32: acc = fmaf(z_0, W[0][c], 0); acc = fmaf(z_i, W[i][c], acc) for
 *                             i = 1 .. Fin - 1 ascending; then acc + bias[c] (skipped when bias is NULL); then, with
 *                             relu, acc < 0 ? 0 : acc (NaN stays NaN).  No sum mixes units: a sample's y is bitwise
 *                             that of the batch = 1 call on a contiguous copy of its columns.
 *   gcn_agg_linear_backward   with gp = relu ? (y <= 0 ? 0 : g) : g  (y: the forward result; NULL allowed without
 *                             relu):  grad_w[i, c] = sum_r sum_j z[r, j * Fin + i] * gp[r, j * Fout + c]  (fp32
 *                             [Fin, Fout]),  grad_b[c] = sum_r sum_j gp[r, j * Fout + c]  (fp32 [Fout], or NULL: not
 *                             formed).  Two stages, all sums in DOUBLE: block b of the sweep owns the units
 *                             [b * R, min((b + 1) * R, M)), its wavefront w the units [b * R + 16 * P * w,
 *                             b * R + 16 * P * (w + 1)) of them; a lane owns one column and the wavefront's units of
 *                             one parity, ascending; the two parities are added, then the 4 wavefronts in order, into
 *                             row b of `partials` (Fin * Fout doubles of grad_w row-major, then Fout of grad_b).  The
 *                             finishing launch adds the rows in block order 0, 1, ... and rounds once to fp32.  No
 *                             atomics: bitwise reproducible, whichever block ran first.  g, z (and y) are read once.
 * There is no input-gradient sweep: a layer whose input needs a gradient is evaluated as A·(X·W).
 * SHAPE RULE: 1 <= n_rows <= 2^40, Fin in {4, 8, ..., 32}, Fout = 32, 1 <= batch <= 65535 (else GCN_E_BADARG, as a
 * NULL z, weight, y / g, grad_w, or y with relu); z, y, g, weight and bias 16-byte aligned, grad_w and grad_b 4-byte,
 * partials 8-byte (GCN_E_ALIGN).
 * Scratch of gcn_agg_linear_backward: `partials`, DEVICE double [partial_rows][Fin * Fout + Fout], allocated by the
 * caller (NULL, or partial_rows below the query: GCN_E_WORKSPACE), with
 *     gcn_agg_linear_partial_rows = B,
 *     M = n_rows * batch,  P = ceil(M / (64 * 2048)),  R = 64 * P,  B = ceil(M / R)  (<= 2048)
 * and 0 outside the shape rule.
 * (ABI 26, additive.)
 */
int64_t gcn_agg_linear_partial_rows(int64_t n_rows, int64_t Fin, int64_t Fout, int64_t batch);
int gcn_agg_linear_forward(const float *z, const float *weight, const float *bias, float *y, int64_t n_rows,
                           int64_t Fin, int64_t Fout, int64_t batch, int relu, void *stream);
int gcn_agg_linear_backward(const float *g, const float *y, const float *z, int64_t n_rows, int64_t Fin,
                            int64_t Fout, int64_t batch, int relu, float *grad_w, float *grad_b, double *partials,
                            int64_t partial_rows, void *stream);

/*
 * Dense adjacency ingest (pygcn_amd/csrc/gcn_dense.hip): a dense fp32 matrix A [n_rows, n_cols], row pitch lda >=
 * n_cols elements, to CSR — the fork loads its co-visit matrix as a dense [N, N] float tensor (reference
 * pygcn/utils.py:124-131) and never builds a sparse one.  Two sweeps with the caller's scan between them, as
 * gcn_csr_take_rows has it.  All pointers DEVICE; nothing is read by the host.  Row i, entries a_j = A[i * lda + j]:
 *   THE VALUE RULE   GCN_DENSE_NONZERO   keep a  iff  !(a == 0):  -0 and +0 dropped, NaN kept (torch.nonzero's rule);
 *                    GCN_DENSE_GREATER   keep a  iff  a > bound, the ordinary float comparison: NaN dropped.
 *   thr == NULL      entry j is kept iff the value rule holds.
 *   thr != NULL      count_gt must be non-NULL and 1 <= keep <= n_cols.  thr[i] and count_gt[i] are gcn_select_kth's
 *                    answers for window i at kth = keep (A contiguous is exactly its [batch = n_rows, n_rows = n_cols]
 *                    layout).  The selected set S_i is every entry whose key is greater than thr[i], plus the
 *                    lowest-column entries whose key equals it, until S_i has `keep` members; keys compare in the
 *                    selection ORDER above (-0 is +0, every NaN above +inf).  Entry j is kept iff j is in S_i AND the
 *                    value rule holds: a row keeps at most `keep` entries, and a row with fewer non-zeros than `keep`
 *                    keeps just those.
 *   gcn_dense_to_csr_count   row_count[i] (int32 [n_rows]) = the number of kept entries of row i.
 *   gcn_dense_to_csr_fill    writes the kept entries of row i at rowptr[i] + 0, 1, ... in ASCENDING COLUMN ORDER:
 *                            col int32, val the stored float bit for bit (a NaN keeps its payload, nothing is
 *                            canonicalised).  rowptr [n_rows + 1] is the caller's exclusive scan of row_count (int32,
 *                            or int64 with rowptr_is64).  Nothing outside [0, rowptr[n_rows]) is written, and nothing
 *                            outside row i's slots for row i, whatever rowptr says.
 * One 256-thread block per row, rows grid-stride from a grid of at most GCN_DENSE_SWEEP_ROWS blocks, so any n_rows
 * below 2^31 runs; a row is read in chunks of 1024 columns, four per lane as one 16-byte access where A + i * lda is
 * 16-byte aligned, else element by element; the fill ranks a chunk's kept entries by ballots and popcounts (one
 * barrier per chunk).  A matrix of few very long rows under-fills the chip.  No atomics: two runs give the same bytes.
 * GCN_E_BADARG: n_rows < 0, n_cols < 1 or n_cols >= 2^31, lda < n_cols, an unknown rule, thr without count_gt, keep
 * outside [1, n_cols] with thr, a NULL array with n_rows > 0.  GCN_E_ALIGN: a pointer that is not 4-byte aligned (an
 * int64 rowptr: 8-byte).  Checked before any launch; n_rows = 0 launches nothing and returns 0.
 * (ABI 26, additive.)
 */
#define GCN_DENSE_NONZERO 0
#define GCN_DENSE_GREATER 1
#define GCN_DENSE_SWEEP_ROWS 8192   /* rows that one sweep of the grid covers */
int gcn_dense_to_csr_count(const float *A, int64_t lda, int64_t n_rows, int64_t n_cols, int rule, float bound,
                           const float *thr, const int32_t *count_gt, int64_t keep, int32_t *row_count, void *stream);
int gcn_dense_to_csr_fill(const float *A, int64_t lda, int64_t n_rows, int64_t n_cols, int rule, float bound,
                          const float *thr, const int32_t *count_gt, int64_t keep, const void *rowptr, int rowptr_is64,
                          int32_t *col, float *val, void *stream);

/*
 * Neighbour sampling (pygcn_amd/csrc/gcn_sample.hip; CSRGraph.sample_neighbors): at most K = fanout of the stored
 * entries of every row of a CSR matrix, as a CSR matrix of its own — the fan-out of GraphSAGE-style training, DropEdge
 * as its special case.  A per-row segmented select with no sort, NO WORKSPACE and no allocation; all pointers DEVICE,
 * nothing is read by the host.  Output row r is made from source row s = rows[r] (rows: int64 [m], each in
 * [0, n_rows) — the CALLER'S duty, it is not checked — any order, repeats allowed), or s = r when rows is NULL.  With
 * d the number of stored entries of row s:
 *   d <= K    the row is copied.
 *   d >  K    exactly K entries are kept: those with the K largest 32-bit KEYS, compared as unsigned integers; on
 *             equal keys the entry stored earlier wins.
 * Kept entries come out in their stored order (ascending columns stay ascending), the columns unchanged, the values
 * bit for bit the stored ones unless rescale is set.  rowptr_out [m + 1] (int32, or int64 with out_is64) is SUPPLIED
 * by the caller: the exclusive scan of min(d, K), which needs no pass over the entries; col_out / val_out have
 * rowptr_out[m] entries.  Nothing outside a row's own slots is written for that row, whatever rowptr_out says.
 *   THE RANDOM WORD of the entry at index e of the SOURCE arrays col / val:
 *       w(e) = Philox4x32-10(counter = (lo32(e >> 2), hi32(e >> 2), draw_stream, 2), key = (lo32(seed), hi32(seed)))[e & 3]
 *   — counter word 3 = 2 keeps the stream apart from the dropout's (0) and the race keys' (1).  It depends on
 *   (seed, draw_stream, e) only: sampling the rows `rows` gives, bit for bit, the rows `rows` of the sample of the
 *   whole matrix, and no launch shape can change a draw.
 *   THE KEY, by mode:
 *       GCN_SAMPLE_UNIFORM     w(e): every K-subset of the row is equally likely.  val takes no part in the choice.
 *       GCN_SAMPLE_WEIGHT      the selection-order key ("Vertex selection" above: -0 is +0, NaN above +inf) of
 *                              fp32(double(val) / E), E = -log((w(e) + 0.5) * 2^-32) — the race key of gcn_race_keys:
 *                              K draws without replacement with probability proportional to the value
 *                              (Plackett-Luce).  Values must be finite and >= 0, which is NOT checked.  A zero value
 *                              has the key of +0: zeros are taken last, lowest position first.
 *       GCN_SAMPLE_STRONGEST   the selection-order key of val: deterministic, seed and draw_stream are ignored.
 *   keep_diagonal (0 / 1)   the first stored entry of row s with col == s is kept ahead of the key order and counts as
 *                           one of the K; the other K - 1 are the largest keys of the remaining entries.
 *   rescale                 GCN_SAMPLE_RESCALE_NONE leaves the values alone.  GCN_SAMPLE_RESCALE_SUM, in rows with
 *                           d > K only: S = the sum of all stored values of the row, S' = that of the kept ones, both in
 *                           double; ratio = fp32(S / S'), formed in double and rounded once; every kept value is
 *                           multiplied by ratio in fp32.  A row whose ratio is not finite (S' = 0) keeps its values.
 *                           A row-normalised matrix keeps its row sums (the GraphSAGE mean).  The double additions run
 *                           in a fixed order — a lane's entries in stored order, then the lanes, then the waves — so
 *                           two runs give the same bytes; a sum in another order can move ratio by one fp32 step only
 *                           where S / S' lies within a few double steps of an fp32 rounding boundary.
 * Rows of up to GCN_SAMPLE_WAVE_ROW_MAX entries take one wavefront each, the row in registers (a grid of at most
 * GCN_SAMPLE_WAVE_SWEEP_ROWS wavefronts strides over the rows); longer rows take one workgroup each, which computes the
 * keys again in each of its passes.  A row holds fewer than 2^32 entries.  No float atomics.
 * GCN_E_BADARG, before any launch and without a device: fanout < 1, an unknown mode or rescale, m < 0 or m > 2^40, a
 * NULL array other than rows with m > 0.  GCN_E_ALIGN: rows or a 64-bit row pointer not 8-byte aligned, another array
 * not 4-byte aligned.  m = 0 launches nothing and returns 0.
 * (ABI 26, additive.)
 */
#define GCN_SAMPLE_UNIFORM 0
#define GCN_SAMPLE_WEIGHT 1
#define GCN_SAMPLE_STRONGEST 2
#define GCN_SAMPLE_RESCALE_NONE 0
#define GCN_SAMPLE_RESCALE_SUM 1
#define GCN_SAMPLE_WAVE_ROW_MAX 253         /* the longest row that one wavefront holds in registers */
#define GCN_SAMPLE_WAVE_SWEEP_ROWS 65536    /* rows that one sweep of the row-per-wavefront grid covers */
int gcn_csr_sample_rows(const void *rowptr, int rowptr_is64, const int32_t *col, const float *val, const int64_t *rows,
                        int64_t m, int64_t fanout, int mode, uint64_t seed, uint32_t draw_stream, int keep_diagonal,
                        int rescale, const void *rowptr_out, int out_is64, int32_t *col_out, float *val_out,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GCN_SPMM_H */
