/* bsmm_adafactor.h -- C ABI of the Adafactor step of libbsmm_hip.so: factored second moments for a dense matrix, a vector and a block-sparse
 * tensor.  Same boundary rules as bsmm_optim.h (which this header includes for bsmm.h's BSMM_F32 / BSMM_F16 / BSMM_BF16 and BSMM_ERR_*):
 * every pointer is a device pointer owned by the caller, nothing is allocated, a call only enqueues work on `stream` (a hipStream_t) and
 * returns; 0 = ok, > 0 = a hipError_t, < 0 = BSMM_ERR_*; no environment variables, no global state, no atomics, no host sync; kernel choice
 * is a function of the arguments only (sizes and pointer alignment).  Every argument is checked before anything is launched.  BSMM_VERSION
 * (bsmm.h) is unchanged: these are new symbols, no existing layout moves.
 *
 * What it replaces (paths relative to the reference, openai/blocksparse): ops "Adafactor2d" / "Adafactor1d", blocksparse/optimize.py:118-191,
 * src/optimize_op_gpu.cu:8-362 -- there four kernels, a full-size fp32 scratch for the normalised gradient and atomic adds for the mean of
 * rv and for the RMS; here no scratch of the tensor's size, no atomics, and a block form the reference does not have.
 *
 * Arithmetic: fp32 throughout, IEEE square root and division; pre() and the "skip this step" sentinel are those of bsmm_adam.
 *     g' = pre(g) * (grad_scale * norm_scale)             s = fma(g', g', epsilon)
 *     moment(old, mean) = fma(decay, old, (1 - decay) * mean)             with 1 - decay rounded to fp32 on the host
 *
 *   2-d form (bsize 0, rows = C > 1, cols = K; rv fp32 [C], cv fp32 [K]):
 *     rv_c <- moment(rv_c, (sum_k s_ck) * inv_K)          cv_k <- moment(cv_k, (sum_c s_ck) * inv_C)
 *     m = (sum_c rv_c) * inv_C                             over the new rv
 *     x_ck = g'_ck * ((1 / sqrt(rv_c / m)) * (1 / sqrt(cv_k)))
 *     rate = lr / max(sqrt((sum_ck x^2) * inv_CK) / clip_thresh, 1)       p <- fma(-rate, x, p)
 *     inv_K, inv_C, inv_CK: 1 / K, 1 / C, 1 / (C K) computed in double on the host and rounded once to fp32.
 *   1-d form (bsize 0, rows == 1; cv fp32 [K], rv not read):
 *     cv_k <- moment(cv_k, s_k)          x_k = g'_k / sqrt(cv_k)          rate and p as above with inv_K
 *   block form (bsize 8 / 16 / 32 / 64, rows = blocks, cols = bsize^2; rv and cv fp32 [blocks][bsize]):
 *     every block is a 2-d problem of its own with C = K = bsize and its own m (inv_C = inv_K = 1 / bsize, exact): the state is 2 / bsize
 *     of Adam's.  The sum of x^2 and the rate are one value for the tensor, over the live blocks only:
 *     rate = lr / max(sqrt((sum x^2) * (1 / ((float)live * (float)bsize^2))) / clip_thresh, 1), live = the number of blocks whose gate is
 *     not 0, an exact integer sum on the device.  A block whose gate is exactly 0 is neither read nor written in any tensor and does
 *     not count.  If every gate is 0, nothing is stored.
 *
 * *norm_scale == 0 stores nothing in param, cv, rv or param16 (the workspace may be written).  param16, where given, is written wherever
 * param is: param rounded once to nearest-even.  lr and decay are host scalars: a captured step replays with the values it was captured
 * with (the limit bsmm_adam has for lr).
 *
 * Sums.  Every partial sum has a workspace slot of its own; every slot a call reads, that same call has stored (no memset, no dependence
 * on earlier contents).  Partials are added in a fixed order that depends on rows, cols, bsize and the access path only (the 16-byte path
 * when param, cv, grad, param16 and the workspace are 16-byte aligned and cols % 4 == 0, the element path otherwise): the same arguments
 * give the same bits.  No sum of more than 64 terms runs as one sequential fp32 chain -- lane partials, the wave reduction, slots, a
 * fixed-order final sum -- while rows <= 8192, cols <= 4 Mi, rows * cols <= 2^32 and blocks <= 256 Ki; beyond that the strided chains
 * grow in proportion to the size (blocksparse_amd/csrc/bsmm_adafactor_kernels.h spells out every order).
 * Launches per call: 4 (2-d form), 2 (1-d form), 2 (block form).  grad is read 3 / 2 / 2 times, param read and written once. */
#ifndef BSMM_ADAFACTOR_H_
#define BSMM_ADAFACTOR_H_

#include "bsmm_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bsmm_adafactor_args {
    float* param;             /* fp32 [rows * cols] */
    float* cv;                /* fp32 [cols]; block form: [rows * bsize] */
    float* rv;                /* fp32 [rows]; block form: [rows * bsize]; not read when bsize == 0 and rows == 1 */
    const void* grad;         /* [rows * cols] in grad_dtype */
    void* param16;            /* optional: [rows * cols] in param16_dtype */
    const float* gate;        /* optional: fp32 [rows] (one per block); NULL when bsize == 0 */
    const float* norm_scale;  /* optional: one fp32 on the device */
    void* workspace;          /* >= bsmm_adafactor_workspace_bytes(rows, cols, bsize) bytes, 4-byte aligned */
    size_t workspace_bytes;
    void* stream;             /* hipStream_t */
    size_t rows;              /* >= 1; block form: the number of blocks */
    size_t cols;              /* >= 1; block form: bsize^2 */
    int32_t bsize;            /* 0 (dense) / 8 / 16 / 32 / 64 */
    int32_t grad_dtype;       /* BSMM_F32 / BSMM_F16 / BSMM_BF16 */
    int32_t param16_dtype;    /* BSMM_F16 / BSMM_BF16; read only when param16 != NULL */
    int32_t zero_infs;
    int32_t zero_nans;
    float lr;
    float decay;
    float epsilon;
    float clip_thresh;        /* > 0 */
    float grad_scale;
    float saturate;           /* 0 = off */
} bsmm_adafactor_args;

int bsmm_adafactor(const bsmm_adafactor_args* a);

/* Host arithmetic: non-decreasing in rows and in cols, a multiple of 4; 0 for bad sizes (a zero, an unsupported bsize, cols != bsize^2, more
 * than 2^31 - 1 blocks, a size that overflows).  About rows * cols / 32 floats for the 2-d form (the column partials of each slab of 32
 * rows), 9 KiB for the 1-d form, 9 KiB + one float per block for the block form. */
size_t bsmm_adafactor_workspace_bytes(size_t rows, size_t cols, int32_t bsize);

#ifdef __cplusplus
}
#endif
#endif /* BSMM_ADAFACTOR_H_ */
