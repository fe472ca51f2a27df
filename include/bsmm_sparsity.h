/* bsmm_sparsity.h -- C ABI of the dynamic-sparsity operators of libbsmm_hip.so: what decides which blocks of a block-sparse layer to
 * drop and which absent blocks to add.  Same boundary rules as bsmm.h (which this header includes for BSMM_F32 / BSMM_F16 / BSMM_BF16
 * and the BSMM_ERR_* codes): every pointer is a device pointer owned by the caller unless said otherwise, nothing is allocated, every
 * call only enqueues work on `stream` (a hipStream_t) and returns; 0 = ok, > 0 = a hipError_t, < 0 = BSMM_ERR_*; no environment
 * variables, no global state, kernel choice is a function of the arguments only (sizes and pointer alignment).  Arguments are checked
 * before anything is launched.
 *
 * What each entry point replaces (paths relative to the reference, openai/blocksparse):
 *   bsmm_block_norm             <- op "BlocksparseNorm"            blocksparse/optimize.py:315-317, src/optimize_op_gpu.cu:890-980
 *   bsmm_block_l2_decay         <- op "BlocksparseL2Decay"         blocksparse/optimize.py:301-307, src/optimize_op_gpu.cu:793-886
 *   bsmm_block_threshold_prune  <- op "BlocksparseThresholdPrune"  blocksparse/optimize.py:337-341, src/optimize_op_gpu.cu:1005-1098
 *   bsmm_block_prune            <- op "BlocksparsePrune"           blocksparse/optimize.py:326-335, src/optimize_op_gpu.cu:984-1001
 *                                  (the host computes `keep`, src/optimize_op.cc:651-670)
 *   bsmm_feature_reduce + bsmm_reduced_dw
 *                               <- op "BlocksparseReducedDW" ("block reduced full param gradient for use in network growth"):
 *                                  blocksparse/matmul.py:556-609, src/blocksparse_matmul_op.cc:591-773 (BlocksparseFeatureReduceCN / NC,
 *                                  then hGemmTN / hGemmNT), test/blocksparse_reduced_dw_test.py
 *
 * Weights are W [blocks][bsize][bsize] with bsize 8 / 16 / 32 / 64 in fp32, fp16 or bf16; norms and gates are fp32 [blocks].
 * norm_type: 0 = max |w|, 1 = sqrt(sum w^2) (fp32 sum).
 */
#ifndef BSMM_SPARSITY_H_
#define BSMM_SPARSITY_H_

#include "bsmm.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { BSMM_NORM_MAX = 0, BSMM_NORM_L2 = 1 };

/* norm_out[b] = norm of block b.  The max norm of a 16-bit tensor is exact. */
int bsmm_block_norm(const void* w, float* norm_out, int32_t blocks, int32_t bsize, int32_t dtype, int32_t norm_type, void* stream);

/* Group lasso, in place:  w_b -= w_b * min(rate / sqrt(sum w_b^2 + epsilon), 1)  in fp32, rounded once to the storage type.
 * gate may be NULL; with a gate, a block whose gate is exactly 0 is neither read nor written. */
int bsmm_block_l2_decay(void* w, const float* gate, float rate, float epsilon, int32_t blocks, int32_t bsize, int32_t dtype, void* stream);

/* gate[b] = norm_b < threshold ? 0 : 1 for EVERY block: a block that was gated off comes back when its norm is at or above the
 * threshold, as in the reference. */
int bsmm_block_threshold_prune(const void* w, float* gate, float threshold, int32_t norm_type, int32_t blocks, int32_t bsize, int32_t dtype,
                               void* stream);

/* gate[idx[i]] = i < keep ? 1 : 0 for i < blocks.  idx: int32 [blocks], the block ids by descending norm.  0 <= keep <= blocks;
 * an id outside 0 .. blocks - 1 is skipped. */
int bsmm_block_prune(float* gate, const int32_t* idx, int32_t blocks, int32_t keep, void* stream);

/* Stage 1 of the block-reduced weight gradient: out[fb][p][n] = max-abs (norm_type 0) or l2 norm (1) over the bsize features of feature
 * block fb of activation tensor xs[p] at minibatch column n.
 *   xs      HOST array of pcount (1..8) device pointers; each tensor is (F, N) row-major for axis 0 and (N, F) for axis 1
 *   out     [F / bsize][pcount][N] for BOTH axes (the contraction index p * N + n of stage 2 is contiguous), in a 16-bit type:
 *           fp16 in -> fp16 out, bf16 in -> bf16 out, fp32 in -> bf16 out (one kernel family for stage 2, and the result is a growth
 *           heuristic: an upper bound of the block norm, not an estimate of it).  Max-abs of 16-bit inputs is exact; l2 is an fp32 sum of
 *           squares, a square root and one rounding.
 *   bsize   8 / 16 / 32 on both axes, 64 on axis 1.  F % bsize == 0.  axis 0: N % 8 == 0; axis 1: any N >= 1.
 * One read of the activations, 16 bytes per lane and load when the tensors (and out) are 16-byte aligned; any alignment is accepted. */
int bsmm_feature_reduce(const void* const* xs, int32_t pcount, void* out, int32_t F, int32_t N, int32_t bsize, int32_t axis, int32_t dtype,
                        int32_t norm_type, void* stream);

/* Stage 2:  dw[CB][KB] (fp32, row-major) = scale * x_red . y_red^T  [+ dw when accumulate != 0]
 *   x_red [CB][contraction], y_red [KB][contraction]: stage-1 outputs (contraction = pcount * N), red_dtype BSMM_F16 or BSMM_BF16.
 *   CB, KB >= 1, even or odd.
 * The contraction is cut into slices, one wave per (32 x 32 tile of dw, slice); the slices' fp32 partial sums go to `workspace`
 * (>= bsmm_reduced_dw_workspace_bytes(CB, KB, contraction) bytes) and a second launch adds them in ascending order: no atomics, the same
 * arguments give the same bits.  scale == 0 launches nothing and leaves dw as it is (src/blocksparse_matmul_op.cc:752). */
int bsmm_reduced_dw(const void* x_red, const void* y_red, float* dw, int32_t CB, int32_t KB, int32_t contraction, float scale,
                    int32_t accumulate, int32_t red_dtype, void* workspace, size_t workspace_bytes, void* stream);

/* Host arithmetic: non-decreasing in the contraction length; 0 for non-positive sizes. */
size_t bsmm_reduced_dw_workspace_bytes(int32_t CB, int32_t KB, int32_t contraction);

#ifdef __cplusplus
}
#endif
#endif /* BSMM_SPARSITY_H_ */
