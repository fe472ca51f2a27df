/* bsmm_ew.h -- C ABI of the epilogue of a block-sparse layer in libbsmm_hip.so: bias + activation (none / ReLU / fast-GELU) with gradients
 * in BOTH activation layouts of the matmul, a stateless and bit-reproducible dropout mask of 1 bit per element, the mask's application, and
 * the fused pair bias -> activation -> dropout -> (+ residual) forward and backward.  Same boundary rules as bsmm_norm.h (bsmm.h is included
 * for BSMM_F32 / BSMM_F16 / BSMM_BF16 and the BSMM_ERR_* codes): every pointer is a device pointer owned by the caller, nothing is
 * allocated, every call only enqueues work on `stream` (a hipStream_t) and returns; 0 = ok, > 0 = a hipError_t, < 0 = BSMM_ERR_*; no
 * environment variables, no global state, kernel choice is a function of the arguments only (sizes and pointer alignment).  Arguments are
 * checked before anything is launched.
 *
 * What each entry point replaces (paths relative to the reference, openai/blocksparse):
 *   bsmm_bias_act / _grad       <- ops "BiasRelu" / "BiasReluGrad" / "BiasGrad"   blocksparse/ewops.py:300-370, src/ew_op_gpu.cu:918-1100,
 *                                  fast_gelu = the reference's _swish with alpha 1.702 (src/ew_op_gpu.h:947)
 *   bsmm_dropout_mask / _apply  <- ops "GenDropoutMask" / "ApplyDropoutMask" / "Dropout"   blocksparse/ewops.py:372-420, src/ew_op_gpu.cu:687-800
 *   bsmm_bias_act_dropout / _grad   the chain the reference's transformer runs after every matmul (examples/transformer/enwik8.py:128-146)
 *                                  as one launch each way.
 *
 * Shapes: K features, N = product of all other dims; axis 0: x is (K, N) row-major, axis 1: x is (N, K) row-major.  x, y, dy, dx, residual:
 * `dtype`.  b, db: fp32 [K].  K * N < 2^31.
 *
 * Element-wise, in fp32:   z = x + b[k]
 *   act 0: v = z          act 1 (ReLU): v = max(z, 0)          act 2 (fast-GELU): v = z * s,  s = 1 / (1 + exp(-1.702 z))
 *   dropout:  v = kept ? v * scale : 0          residual:  v = v + residual          then ONE rounding to the storage type.
 * The multiply by scale and the add of the residual are separate fp32 operations (never one fused multiply-add): an fp32 call of the fused
 * forward stores the bits the sequence bsmm_bias_act, bsmm_dropout_apply, add stores.
 * Backward:  g = kept ? dy * scale : 0 (dropout), then  act 0: dx = g;  act 1: dx = z > 0 ? g : 0;  act 2: dx = g * (s + 1.702 z s (1 - s)),
 * finite for every finite z;  db[k] = sum_n dx, of the fp32 values before they are rounded.
 *
 * The dropout mask: ceil(n / 32) words of 32 bits, bit (i % 32) of word (i / 32) belongs to element i of the contiguous tensor (the
 * reference's packing, src/ew_op_gpu.cu:760-764), 1 = kept; the pad bits of the last word are 0.  Its definition is fixed so that a host can
 * reproduce it (blocksparse_amd.ewops.dropout_mask_test does): `state` points to two uint64 on the device, {seed, offset}; element i belongs
 * to generator call c = i / 8;
 *     w[0..3] = Philox4x32-10(counter = (c_lo, c_hi, offset_lo, offset_hi), key = (seed_lo, seed_hi))
 *     r       = (w[(i % 8) / 2] >> (16 * (i % 2))) & 0xffff;        kept iff r < threshold,  0 <= threshold <= 65536.
 * The mask depends on seed, offset, threshold and n only: not on the grid, the dtype, the axis or the kernel that wrote it.  No call changes
 * `state`; a caller who wants another mask from the next call advances the offset (blocksparse_amd.ewops does, as device work on the
 * stream, so that a captured step draws a fresh mask on every replay).
 *
 * Sums that cross workgroups (db on axis 1 always; on axis 0 when a row of N is cut over workgroups) go through partials in `workspace` and
 * a second stage that adds them in a fixed order: no floating-point read-modify-write to memory, the same arguments give the same bits.
 * The 16-bytes-per-lane path runs when the activations are 16-byte aligned and the contiguous run allows it -- N % 8 == 0 on axis 0,
 * K % 8 == 0 (and b 16-byte aligned) on axis 1 -- an element path covers every other size and pointer.
 */
#ifndef BSMM_EW_H_
#define BSMM_EW_H_

#include "bsmm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSMM_ACT_NONE 0
#define BSMM_ACT_RELU 1
#define BSMM_ACT_FAST_GELU 2

/* `which` of bsmm_ew_workspace_bytes */
#define BSMM_EW_BIAS_ACT 0
#define BSMM_EW_BIAS_ACT_GRAD 1
#define BSMM_EW_BIAS_ACT_DROPOUT 2
#define BSMM_EW_BIAS_ACT_DROPOUT_GRAD 3

typedef struct bsmm_ew_args {
    int32_t K;          /* features                                                                        */
    int32_t N;          /* product of all other dims, >= 1;  K * N < 2^31                                  */
    int32_t axis;       /* 0: x is (K, N) row-major;  1: x is (N, K) row-major                             */
    int32_t dtype;      /* x, y, dy, dx, residual: BSMM_F32 / BSMM_F16 / BSMM_BF16                         */
    int32_t act;        /* BSMM_ACT_*                                                                      */
    int32_t generate;   /* fused forward: 1 = make the mask bits and WRITE mask, 0 = READ mask             */
    int32_t threshold;  /* dropout: kept iff r < threshold, 0 .. 65536 (= round(keep_prob * 65536))        */
    float   scale;      /* dropout: kept values are multiplied by it (= 1 / keep_prob)                     */
    void*   workspace; size_t workspace_bytes;   /* >= bsmm_ew_workspace_bytes(); may be NULL where that is 0 */
    void*   stream;
} bsmm_ew_args;

/* Every call below answers BSMM_ERR_ARG for: args NULL, K / N < 1, K * N >= 2^31, axis not 0 / 1, an unknown dtype or act, a NULL pointer
 * that is not marked optional, and -- the gradients -- a workspace that is too small or not 4-byte aligned.  The dropout calls also for
 * threshold outside 0 .. 65536, generate not 0 / 1 and a mask that is not 4-byte aligned.  generate, threshold and scale are read by the
 * two dropout calls only. */

/* y <- act(x + b) */
int bsmm_bias_act(const void* x, const float* b, void* y, const bsmm_ew_args* args);

/* dx, db <- dy and what the forward kept: act 1 (ReLU) takes the STORED y and masks dy by y > 0 (the reference saves y so that x can be
 * freed, blocksparse/ewops.py:343-346); act 2 takes x and recomputes z.  act 0: x_or_y is not read and may be NULL, and dx may be NULL
 * (dx = dy): only db is produced. */
int bsmm_bias_act_grad(const void* dy, const void* x_or_y, const float* b, void* dx, float* db, const bsmm_ew_args* args);

/* mask[0 .. ceil(n / 32)) <- the bits defined above.  1 <= n < 2^31. */
int bsmm_dropout_mask(uint32_t* mask, const uint64_t* state, int64_t n, int32_t threshold, void* stream);

/* y[i] <- kept(i) ? x[i] * scale : 0, one fp32 multiply and one rounding; forward and backward of a dropout.  1 <= n < 2^31. */
int bsmm_dropout_apply(const void* x, const uint32_t* mask, void* y, int64_t n, float scale, int32_t dtype, void* stream);

/* y <- dropout(act(x + b)) [+ residual].  generate 1: the kernel makes the bits from `state` and writes all ceil(K N / 32) words of mask;
 * generate 0: it reads mask (the recompute path) and `state` may be NULL.  residual may be NULL.  With act 0, b may be NULL (no bias: a
 * plain dropout that makes its mask in the same launch). */
int bsmm_bias_act_dropout(const void* x, const float* b, const void* residual, const uint64_t* state, uint32_t* mask, void* y,
                          const bsmm_ew_args* args);

/* dx, db <- dy, x, b, mask.  ReLU masks by z > 0 with z = x + b recomputed in fp32 (y no longer tells).  The gradient of the residual is dy
 * itself and needs no kernel. */
int bsmm_bias_act_dropout_grad(const void* dy, const void* x, const float* b, const uint32_t* mask, void* dx, float* db,
                               const bsmm_ew_args* args);

/* Host arithmetic only: bytes of workspace the call `which` (BSMM_EW_*) needs.  Reads K, N and axis; 0 for bad arguments and for the two
 * forward calls; non-decreasing in K and in N. */
size_t bsmm_ew_workspace_bytes(const bsmm_ew_args* args, int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* BSMM_EW_H_ */
