/* bsmm_select.h -- C ABI of the fused row selection in libbsmm_hip.so: activation sparsity along the last axis of a tensor.  Keep the k
 * largest scores of a row (rectified top-k, top-k softmax; k = K is the plain masked softmax) or the activations above mean + alpha * sigma
 * (sparse ReLU), one launch each way.  Same boundary rules as bsmm_lstm.h (bsmm.h is included for BSMM_F32 / BSMM_F16 / BSMM_BF16 and the
 * BSMM_ERR_* codes): every pointer is a device pointer owned by the caller, nothing is allocated, every call only enqueues work on `stream`
 * (a hipStream_t) and returns; 0 = ok, > 0 = a hipError_t, < 0 = BSMM_ERR_*; no environment variables, no global state, no atomics, kernel
 * choice is a function of the arguments only (sizes and pointer alignment).  Arguments are checked before anything is launched.
 *
 * What the entry points replace (paths relative to the reference, openai/blocksparse):
 *   bsmm_rectified_top_k        <- op "RectifiedTopK"                               blocksparse/transformer.py:498-549
 *   bsmm_masked_top_k_softmax   <- ops "MaskedTopKSoftmax", "MaskedSoftmax"         blocksparse/transformer.py:552-649
 *   bsmm_masked_softmax_grad    <- op "MaskedSoftmaxGrad"                           blocksparse/transformer.py:588-656
 *   bsmm_sparse_relu            <- sparse_relu                                      blocksparse/lstm.py:103-117
 *   bsmm_select_relu_grad       <- "EwDxDzza" with the ReLU rule, the gradient of the first and the last
 *   (kernels: src/transformer_op_gpu.cu:19-688.)  Not here: a sorted top_k that returns values and indices, and the transposes.
 *
 * Shapes: x, y, dy, dz, dx are (R, K) row-major, rows along the last axis; 1 <= K <= BSMM_SELECT_MAX_K, R * K < 2^31.
 * mask: fp32, `mask_rows` rows of K; row r of x reads mask row r % mask_rows, mask_rows divides R.  NULL: no mask (mask_rows is ignored).
 * The mask is a float that multiplies; an element whose mask value is 0 is "masked".
 *
 * All arithmetic is fp32, every stored value is rounded once.
 *
 * Scores.  v = (x * m) * scale, two fp32 multiplications in that order, never contracted; without a mask v = x * scale; for
 * bsmm_rectified_top_k v = x.
 *
 * Order.  ONE total order decides every selection: value descending, then index ascending.  -0.0 counts as +0.0.  A NaN ranks above +inf
 * (the rule of torch.topk), so a NaN is selected and shows in its own row only.  Masked elements rank below every unmasked one, by index
 * among themselves.  The selected set S is the first k elements of a row in that order: the result is a function of the arguments only,
 * same arguments, same bits, on every path.  (The reference's bitonic network is not stable; its result on ties depends on the launch.)
 *
 * rectified top-k.   base = max(v_(k), 0) with `rebase` (v_(k): the k-th value in the order; a NaN there counts as 0), else 0.
 *                    y_i = (v_i < base ? base : v_i) - base for i in S, 0 elsewhere.
 * top-k softmax.     p_i = exp(v_i - v_max) / sum_{j in S, unmasked} exp(v_j - v_max) for unmasked i in S (v_max: the largest unmasked
 *                    score), exactly 0 for every other element -- also for a masked element that fewer than k unmasked ones pulled into
 *                    S.  A row with no unmasked element stores zeros (the reference would store 1 / k there: this differs).  The sum runs in
 *                    a fixed order that depends on K only: lane sums in index order, a butterfly over the wave, waves in ascending order.
 *                    k == K is the plain (masked) softmax.
 * its gradient.      dx = (dy - sum_j dy_j * y_j) * y * m * scale from the STORED y (m = 1 without a mask): the zeros outside S make it
 *                    right for top-k.
 * sparse ReLU.       mean = sum(x) / K;  var = sum((x - mean)^2) / K, the population variance, in two passes over the registers -- never
 *                    E[x^2] - mean^2;  cut = mean + alpha * sqrt(var);  y = max(x - cut, 0).
 * ReLU-rule gradient dx = y > 0 ? dz : 0 (the cutoff and the base count as constants, as in the reference).
 *
 * Kernel paths (bsmm_select_path; thresholds below).  A row never leaves its workgroup and is read from memory once, into registers.
 *   K <= BSMM_SELECT_WAVE8_MAX      a wave per row, 8 elements per lane, four rows per workgroup, no LDS, no barrier
 *   K <= BSMM_SELECT_WAVE16_MAX     a wave per row, 16 elements per lane
 *   K <= BSMM_SELECT_GROUP2_MAX     a workgroup of two waves per row, 16 elements per lane, counts and sums cross the waves through LDS
 *   K <= BSMM_SELECT_MAX_K          a workgroup of four waves per row
 * Each with 16-byte accesses when every pointer is 16-byte aligned and K is a multiple of 8 (4 in fp32), by element accesses otherwise.
 * Both forms give a lane the same elements, so they store the same bits.
 */
#ifndef BSMM_SELECT_H_
#define BSMM_SELECT_H_

#include "bsmm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSMM_SELECT_WAVE8_MAX 512
#define BSMM_SELECT_WAVE16_MAX 1024
#define BSMM_SELECT_GROUP2_MAX 2048
#define BSMM_SELECT_MAX_K 4096

/* bsmm_select_path: 2 * geometry + (1 for the 16-byte form) */
#define BSMM_SELECT_PATH_WAVE8 0
#define BSMM_SELECT_PATH_WAVE16 2
#define BSMM_SELECT_PATH_GROUP2 4
#define BSMM_SELECT_PATH_GROUP4 6

typedef struct bsmm_select_args {
    int32_t R;            /* rows, >= 1;  R * K < 2^31                                                        */
    int32_t K;            /* row length, 1 .. BSMM_SELECT_MAX_K                                               */
    int32_t k;            /* elements kept per row, 1 .. K (the two top-k calls; ignored by the others)       */
    int32_t mask_rows;    /* rows of the mask, >= 1 and a divisor of R (read when mask != NULL)               */
    int32_t dtype;        /* x, y, dy, dz, dx: BSMM_F32 / BSMM_F16 / BSMM_BF16                                */
    int32_t rebase;       /* bsmm_rectified_top_k: subtract max(v_(k), 0)                                     */
    float   scale;        /* the softmax calls                                                                */
    float   alpha;        /* bsmm_sparse_relu                                                                 */
    void*   stream;
} bsmm_select_args;

/* Every call answers BSMM_ERR_ARG for: args NULL, R / K < 1, R * K >= 2^31, an unknown dtype, a NULL pointer that is not marked optional,
 * k < 1 or k > K where k is read, and with a mask mask_rows < 1 or not a divisor of R.  A K above BSMM_SELECT_MAX_K in otherwise valid
 * arguments answers BSMM_ERR_UNSUPPORTED (bsmm_select_relu_grad is element-wise and takes any K). */

/* the path for rows of K elements: BSMM_SELECT_PATH_* + 1 when `aligned` (every pointer 16-byte aligned) and K allows 16-byte accesses */
int bsmm_select_path(int K, int dtype, int aligned);

/* y <- x */
int bsmm_rectified_top_k(const void* x, void* y, const bsmm_select_args* args);

/* y <- x [, mask] */
int bsmm_masked_top_k_softmax(const void* x, const float* mask /* or NULL */, void* y, const bsmm_select_args* args);

/* dx <- dy, the stored y [, mask] */
int bsmm_masked_softmax_grad(const void* dy, const void* y, const float* mask /* or NULL */, void* dx, const bsmm_select_args* args);

/* y <- x */
int bsmm_sparse_relu(const void* x, void* y, const bsmm_select_args* args);

/* dx <- dz, the stored y */
int bsmm_select_relu_grad(const void* dz, const void* y, void* dx, const bsmm_select_args* args);

#ifdef __cplusplus
}
#endif
#endif /* BSMM_SELECT_H_ */
