/* bsmm_optim.h -- C ABI of the weight-update operators of libbsmm_hip.so: a gated Adam step, a gated exponential moving average and a
 * deterministic two-stage global-norm clip.  Same boundary rules as bsmm.h (which this header includes for BSMM_F32 / BSMM_F16 / BSMM_BF16
 * and the BSMM_ERR_* codes): every pointer is a device pointer owned by the caller, nothing is allocated, every call only enqueues work on
 * `stream` (a hipStream_t) and returns; 0 = ok, > 0 = a hipError_t, < 0 = BSMM_ERR_*; no environment variables, no global state, no
 * atomics, no host sync; kernel choice is a function of the arguments only (sizes and pointer alignment).  Arguments are checked before
 * anything is launched.  BSMM_VERSION (bsmm.h) is unchanged: these are new symbols, no existing layout moves.
 *
 * What each entry point replaces (paths relative to the reference, openai/blocksparse):
 *   bsmm_adam          <- ops "Adam" (apply_adam, apply_adam_gated) and "BlocksparseAdam" (apply_blocksparse_adam, per-block lr_select):
 *                         blocksparse/optimize.py:20-110, src/optimize_op_gpu.cu:453-790 -- three kernels there, one call here
 *   bsmm_ema           <- op "Ema" (plain and gated): blocksparse/optimize.py:231-289, src/optimize_op_gpu.cu (apply_ema / apply_ema_gated)
 *   bsmm_sum_squared + bsmm_clip_norm
 *                      <- op "ClipGlobalNorm": blocksparse/optimize.py:193-228, src/optimize_op_gpu.cu:1102-1238 (reduce_sum_squared with
 *                         atomicRed, then compute_clip_norm).  Here every partial sum has a slot of its own and the order of every addition
 *                         is fixed: the same arguments give the same bits.
 *
 * A block-sparse tensor is [blocks][bsize][bsize] with bsize 8 / 16 / 32 / 64 (size = blocks * bsize^2); gates and lr selects are fp32
 * [blocks].  bsize 0 is a flat tensor of any size >= 1 (biases, embeddings) and takes neither.
 */
#ifndef BSMM_OPTIM_H_
#define BSMM_OPTIM_H_

#include "bsmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One Adam step, in place.  fp32 arithmetic per element, in this order (src/optimize_op_gpu.cu:577-598):
 *   g = grad;  zero_infs: +-Inf -> 0;  zero_nans: NaN -> 0;  saturate != 0: g = clamp(g, +-saturate)
 *   g *= grad_scale * norm_scale;  v = beta2 v + (1 - beta2) g^2;  sigma = sqrt(v)
 *   clip_sigma != 0: g = clamp(g, +-clip_sigma sigma);  m = beta1 m + (1 - beta1) g;  p -= lr m / (sigma + epsilon)
 * with IEEE square root and division.  A block whose gate is exactly 0 is neither read nor written, in any tensor.  Blocks whose
 * lr_select entry is non-zero step with lr_new, the others with lr.  *norm_scale == 0 is the "skip this step" sentinel of
 * bsmm_clip_norm: nothing at all is stored.  param16, where given, is written wherever param is: param rounded once to nearest-even.
 * lr is a host scalar here: a captured step replays with the lr it was captured with.  bsmm_adam_list (bsmm_optim_list.h) reads the rates
 * from a device-resident step state instead, and steps a whole list of tensors in one launch. */
typedef struct bsmm_adam_args {
    float* param;             /* fp32 [size] */
    float* mean;              /* fp32 [size] */
    float* var;               /* fp32 [size] */
    const void* grad;         /* [size] in grad_dtype */
    void* param16;            /* optional: [size] in param16_dtype */
    const float* gate;        /* optional: fp32 [size / bsize^2]; NULL when bsize == 0 */
    const float* lr_select;   /* optional: fp32 [size / bsize^2]; NULL when bsize == 0 */
    const float* norm_scale;  /* optional: one fp32 on the device */
    void* stream;             /* hipStream_t */
    size_t size;              /* elements; a multiple of bsize^2 when bsize != 0 */
    int32_t bsize;            /* 0 (flat) / 8 / 16 / 32 / 64 */
    int32_t grad_dtype;       /* BSMM_F32 / BSMM_F16 / BSMM_BF16 */
    int32_t param16_dtype;    /* BSMM_F16 / BSMM_BF16; read only when param16 != NULL */
    int32_t zero_infs;
    int32_t zero_nans;
    float lr;
    float lr_new;             /* read only when lr_select != NULL */
    float beta1;
    float beta2;
    float epsilon;
    float grad_scale;
    float clip_sigma;         /* 0 = off */
    float saturate;           /* 0 = off */
} bsmm_adam_args;

int bsmm_adam(const bsmm_adam_args* a);

/* e -= (1 - decay) (e - p) in fp32, rounded once to ema_dtype (BSMM_F32 / BSMM_F16 / BSMM_BF16).  param: fp32 [size].  gate (optional, fp32
 * [size / bsize^2]): blocks whose gate is exactly 0 are neither read nor written.  bsize 0: a flat tensor, gate must be NULL. */
int bsmm_ema(void* ema, const float* param, const float* gate, float decay, size_t size, int32_t bsize, int32_t ema_dtype, void* stream);

/* Global norm, stage 1: the fp32 partial sums of (grad_scale * pre(x))^2 over tensor `tensor_idx` of `tensor_cnt`, stored to that tensor's
 * slots of `workspace` (>= bsmm_sum_squared_workspace_bytes(tensor_cnt) bytes, 4-byte aligned).  pre(x): zero_infs / zero_nans / saturate
 * as in bsmm_adam.  x: [size] in dtype.  Every slot of the tensor is stored on every call (no memset, no dependence on earlier contents);
 * slice boundaries and the order of the additions depend on `size` and the access path (16-byte loads when x is 16-byte aligned, element
 * loads otherwise) only. */
int bsmm_sum_squared(const void* x, size_t size, int32_t dtype, float grad_scale, float saturate, int32_t zero_infs, int32_t zero_nans,
                     int32_t tensor_idx, int32_t tensor_cnt, void* workspace, size_t workspace_bytes, void* stream);

/* Host arithmetic: non-decreasing in tensor_cnt; 0 for non-positive counts. */
size_t bsmm_sum_squared_workspace_bytes(int32_t tensor_cnt);

/* Stage 2, one workgroup: lane l adds slots l, l + 256, ... of the tensor_cnt tensors in ascending order, the lanes' sums are added in a
 * fixed order.  *norm_out = sqrt(sum);  *scale_out = clip_norm / max(norm, clip_norm) when the norm is finite, else 0
 * (src/optimize_op_gpu.cu:1215-1229). */
int bsmm_clip_norm(const void* workspace, size_t workspace_bytes, int32_t tensor_cnt, float clip_norm, float* norm_out, float* scale_out,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BSMM_OPTIM_H_ */
