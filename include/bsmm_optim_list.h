/* bsmm_optim_list.h -- C ABI of the tensor-list form of the weight update (include/bsmm_optim.h): a list of tensors, prepared once, that
 * every stage walks in ONE launch, with the step number and the corrected rates resident on the device.  Clip, Adam and the moving
 * average over T tensors are 3T + 1 launches through bsmm_optim.h and at most 5 here, whatever T; a step captured in a graph follows a
 * learning-rate schedule because the rate is read on the device when the step runs.
 *
 * Same boundary rules as bsmm_optim.h: every device pointer is owned by the caller, nothing is allocated, every device call only enqueues
 * work on `stream` (a hipStream_t) and returns; 0 = ok, > 0 = a hipError_t, < 0 = BSMM_ERR_*; no environment variables, no global
 * state, no atomics, no host sync; arguments are checked before anything is launched.  BSMM_VERSION (bsmm.h) is unchanged: these are new
 * symbols, no existing layout moves.
 *
 * Bit rule: for the same inputs and the same fp32 rates, every tensor bsmm_adam_list / bsmm_ema_list write equals bit for bit what
 * bsmm_adam / bsmm_ema write tensor by tensor, and every workspace slot bsmm_sum_squared_list stores equals the slot of the
 * bsmm_sum_squared call on that tensor (so bsmm_clip_norm, unchanged, gives the same norm and scale).
 */
#ifndef BSMM_OPTIM_LIST_H_
#define BSMM_OPTIM_LIST_H_

#include "bsmm_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One row of the list: the tensors of one param, with the optionals of bsmm_adam_args and bsmm_ema.  A row without `ema` takes no
 * part in bsmm_ema_list.  `gate` serves the Adam step and the moving average alike. */
typedef struct bsmm_opt_tensor {
    float* param;             /* fp32 [size] */
    float* mean;              /* fp32 [size] */
    float* var;               /* fp32 [size] */
    const void* grad;         /* [size] in grad_dtype */
    void* param16;            /* optional: [size] in param16_dtype */
    const float* gate;        /* optional: fp32 [size / bsize^2]; NULL when bsize == 0 */
    const float* lr_select;   /* optional: fp32 [size / bsize^2]; NULL when bsize == 0 */
    void* ema;                /* optional: [size] in ema_dtype */
    size_t size;              /* elements; a multiple of bsize^2 when bsize != 0 */
    int32_t bsize;            /* 0 (flat) / 8 / 16 / 32 / 64 */
    int32_t grad_dtype;       /* BSMM_F32 / BSMM_F16 / BSMM_BF16 */
    int32_t param16_dtype;    /* BSMM_F16 / BSMM_BF16; read only when param16 != NULL */
    int32_t ema_dtype;        /* BSMM_F32 / BSMM_F16 / BSMM_BF16; read only when ema != NULL */
} bsmm_opt_tensor;

/* What the host keeps of a built table. */
typedef struct bsmm_opt_list {
    size_t table_bytes;       /* = bsmm_opt_list_bytes(count) */
    int32_t count;            /* rows */
    int32_t adam_grid;        /* workgroups of bsmm_adam_list */
    int32_t ema_grid;         /* workgroups of bsmm_ema_list; 0 when no row has an average */
    int32_t sum_squared_grid; /* workgroups of bsmm_sum_squared_list */
} bsmm_opt_list;

/* The step state, 16 bytes on the device (4-byte aligned).  The caller sets `step` once (the number of steps taken so far) and zeroes
 * the rest; bsmm_opt_advance writes all of it, bsmm_adam_list reads the two rates. */
typedef struct bsmm_opt_state {
    int32_t step;
    float lr_t;
    float lr_new_t;
    int32_t reserved;
} bsmm_opt_state;

/* The settings of bsmm_adam_args that are the same for every row. */
typedef struct bsmm_adam_settings {
    float beta1;
    float beta2;
    float epsilon;
    float grad_scale;
    float clip_sigma;         /* 0 = off */
    float saturate;           /* 0 = off */
    int32_t zero_infs;
    int32_t zero_nans;
} bsmm_adam_settings;

/* Host arithmetic: bytes of the packed table of `count` rows (a multiple of 16); 0 for non-positive or unsupported counts. */
size_t bsmm_opt_list_bytes(int32_t count);

/* Host only, nothing is launched: checks every row with the checks of bsmm_adam, bsmm_ema and bsmm_sum_squared (the first defect's code is
 * returned), decides each row's access path per stage (the 16-byte path only when every pointer the stage touches is 16-byte aligned)
 * and writes the packed table -- the rows, then per stage the prefix sums of the rows' workgroup counts -- into table_host
 * (>= bsmm_opt_list_bytes(count) bytes, else BSMM_ERR_WORKSPACE) and the descriptor into *info.  The caller copies table_bytes bytes to
 * the device (16-byte aligned) once; no launch function copies anything.  The table holds the rows' addresses: a tensor that moves needs a
 * new table. */
int bsmm_opt_list_build(const bsmm_opt_tensor* rows, int32_t count, void* table_host, size_t table_bytes, bsmm_opt_list* info);

/* One workgroup, one active lane: ++state->step;  c = sqrt(1 - beta2^step) / (1 - beta1^step) in double (1 with zero_init_variables);
 * state->lr_t = (float)((double)*lr * c);  state->lr_new_t likewise from *lr_new, or = lr_t when lr_new is NULL.  lr and lr_new are fp32
 * scalars on the device, written by the caller's schedule with ordinary device work. */
int bsmm_opt_advance(bsmm_opt_state* state, const float* lr, const float* lr_new, double beta1, double beta2, int32_t zero_init_variables,
                     void* stream);

/* bsmm_adam for every row in one launch.  The rates are state->lr_t and state->lr_new_t, read on the device; norm_scale (optional, one
 * fp32 on the device) as in bsmm_adam: 0 stores nothing. */
int bsmm_adam_list(const bsmm_opt_list* info, const void* table_dev, const bsmm_opt_state* state, const float* norm_scale,
                   const bsmm_adam_settings* s, void* stream);

/* bsmm_ema for every row that has an average, in one launch (none when there is no such row). */
int bsmm_ema_list(const bsmm_opt_list* info, const void* table_dev, float decay, void* stream);

/* bsmm_sum_squared of every row's grad in one launch: row i stores the slots of tensor i of info->count in `workspace`
 * (>= bsmm_sum_squared_workspace_bytes(info->count) bytes, 4-byte aligned).  bsmm_clip_norm finishes the norm. */
int bsmm_sum_squared_list(const bsmm_opt_list* info, const void* table_dev, float grad_scale, float saturate, int32_t zero_infs,
                          int32_t zero_nans, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BSMM_OPTIM_LIST_H_ */
