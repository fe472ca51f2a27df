/* bsmm_norm.h -- C ABI of the layer norm of libbsmm_hip.so: the normalisation the reference's models put between two block-sparse
 * matmuls, in BOTH activation layouts of the matmul, with the fused ReLU and fp32 gain / bias gradients.  Same boundary rules as
 * bsmm_sparsity.h (bsmm.h is included for BSMM_F32 / BSMM_F16 / BSMM_BF16 and the BSMM_ERR_* codes): every pointer is a device pointer
 * owned by the caller, nothing is allocated, every call only enqueues work on `stream` (a hipStream_t) and returns; 0 = ok, > 0 = a
 * hipError_t, < 0 = BSMM_ERR_*; no environment variables, no global state, kernel choice is a function of the arguments only (sizes and
 * pointer alignment).  Arguments are checked before anything is launched.
 *
 * What each entry point replaces (paths relative to the reference, openai/blocksparse):
 *   bsmm_layer_norm       <- op "LayerNorm"      blocksparse/norms.py:23-56,  src/layer_norm_op.cc:24-170,
 *                                                src/layer_norm_cn_op_gpu.cu (feature axis 0), src/layer_norm_nc_op_gpu.cu (axis 1)
 *   bsmm_layer_norm_grad  <- op "LayerNormGrad"  blocksparse/norms.py:58-67,  src/layer_norm_op.cc:172-330, same two kernel files
 * Semantics are those of the reference's NumPy functions layer_norm_test / layer_norm_grad_test (blocksparse/norms.py:103-180), which do
 * segments on both axes; the reference's kernels want N % 4 == 0 on axis 0 and segments on axis 1 only, this library takes any K >= 1 and
 * N >= 1 on both axes and any pointer alignment.
 *
 * Per segment (a run of K / S features) and per sample, in fp32:
 *   mean = mean of the K / S features,  rstd = 1 / sqrt(biased variance + epsilon)      (variance = mean of squared deviations; it is
 *                                                                                        never computed as E[x^2] - mean^2)
 *   y    = (x - mean) * rstd * g + b,   with relu: max(y, 0) on the fp32 value;  ONE rounding to the storage type
 * Backward, with xhat recomputed from x, mean and rstd:
 *   with relu, dy is first masked by (xhat * g + b) > 0 in fp32 (not by the rounded y)
 *   dg[k] = sum_n dy * xhat,   db[k] = sum_n dy
 *   dx    = (dy * g - (xhat * sum_k(xhat * dy * g) + sum_k(dy * g)) / (K / S)) * rstd         (sums over the segment's features)
 * g, b, dg, db: fp32 [K].  mean, rstd: fp32 [S][N].  x, y, dy, dx: `dtype`, (K, N) row-major for axis 0 and (N, K) for axis 1.
 *
 * Sums that cross workgroups (dg / db, and on axis 0 the per-sample sums of a K that is cut over workgroups) go through per-workgroup
 * partials in `workspace` and a second stage that adds them in a fixed order: no floating-point read-modify-write to memory, the same
 * arguments give the same bits.  The 16-bytes-per-lane path runs when x / y (dy / dx) are 16-byte aligned and the contiguous run allows
 * it -- N % 8 == 0 (16-bit) or N % 4 == 0 (fp32) on axis 0, the same for K / S on axis 1 -- an element path covers the rest.
 */
#ifndef BSMM_NORM_H_
#define BSMM_NORM_H_

#include "bsmm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bsmm_ln_args {
    int32_t K;         /* features (the normalised axis, all segments together)            */
    int32_t N;         /* product of all other dims, >= 1                                  */
    int32_t segments;  /* S >= 1, K % S == 0: each run of K/S features is normalised alone */
    int32_t axis;      /* 0: x is (K, N) row-major;  1: x is (N, K) row-major              */
    int32_t dtype;     /* x, y, dy, dx: BSMM_F32 / BSMM_F16 / BSMM_BF16                    */
    int32_t relu;      /* 0 / 1                                                            */
    float   epsilon;
    void*   workspace; size_t workspace_bytes;   /* >= bsmm_layer_norm_workspace_bytes(); may be NULL where that is 0 */
    void*   stream;
} bsmm_ln_args;

/* y, mean, rstd <- x, g, b.  BSMM_ERR_ARG: a NULL pointer, K / N / segments < 1, K % segments != 0, axis not 0 / 1, an unknown dtype,
 * relu not 0 / 1, a workspace that is too small (or not 4-byte aligned). */
int bsmm_layer_norm(const void* x, const float* g, const float* b, void* y, float* mean, float* rstd, const bsmm_ln_args* args);

/* dx, dg, db <- dy, x, g, b, mean, rstd (mean and rstd as bsmm_layer_norm stored them).  Same checks. */
int bsmm_layer_norm_grad(const void* dy, const void* x, const float* g, const float* b, const float* mean, const float* rstd,
                         void* dx, float* dg, float* db, const bsmm_ln_args* args);

/* Host arithmetic only: bytes of workspace the forward (backward == 0) or the backward call needs.  Reads K, N, segments, axis and dtype;
 * 0 for non-positive sizes or bad arguments; non-decreasing in K and in N. */
size_t bsmm_layer_norm_workspace_bytes(const bsmm_ln_args* args, int32_t backward);

#ifdef __cplusplus
}
#endif
#endif /* BSMM_NORM_H_ */
