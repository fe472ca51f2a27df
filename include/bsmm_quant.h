/* bsmm_quant.h -- C ABI of the simulated float formats in libbsmm_hip.so: round a tensor onto the grid of a format (exponent bits, fraction
 * bits, top exponent) with nearest or stochastic rounding, per tensor or per block of 32 elements, and the statistics that choose the top
 * exponent (saturation share, flush-to-zero share, max, mean and deviation).  Same boundary rules as bsmm_ew.h (bsmm.h is included for
 * BSMM_F32 / BSMM_F16 / BSMM_BF16 and the BSMM_ERR_* codes): every pointer is a device pointer owned by the caller, nothing is allocated,
 * every call only enqueues work on `stream` (a hipStream_t) and returns; 0 = ok, > 0 = a hipError_t, < 0 = BSMM_ERR_*; no environment
 * variables, no global state; arguments are checked before anything is launched; no floating-point read-modify-write to memory.
 *
 * What each entry point replaces (paths relative to the reference, openai/blocksparse):
 *   bsmm_quantize              <- op "Quantize"   blocksparse/quantize.py:74-139, src/quantize_op.cc:57-196, src/quantize_op_gpu.cu:7-101
 *   bsmm_tensor_stats          <- op "LogStats" and QuantizationStats   src/quantize_op.cc:200-305, src/quantize_op_gpu.cu:104-239
 *   bsmm_quant_update_emax     <- the exponent update inside QuantizeOp::Compute (src/quantize_op.cc:137-158), as device work
 *
 * THE FORMAT.  (ebits, fbits, emax, denorm), 1 <= ebits <= 8, 0 <= fbits <= 23 (the counts of src/quantize_op.cc:72-111):
 *   nexp  = 2^ebits - 1 exponent bins, 254 for ebits = 8
 *   e_hi  = clamp(emax, nexp - 127, 127)                            the top binade
 *   s_min = max(e_hi - nexp + 1 - (denorm ? fbits : 0), -125)       the exponent of the smallest step
 *   e_lo  = s_min + (denorm ? fbits : 0)                            the smallest normal binade
 *   max_float = (2 - 2^-fbits) * 2^e_hi
 * The grid: 0;  +- m * 2^(e - fbits) for e_lo <= e <= e_hi and 2^fbits <= m < 2^(fbits + 1);  with denorm also +- m * 2^s_min for
 * 1 <= m < 2^fbits.
 *
 * THE ROUNDING  y = Q(x), integer arithmetic on the fp32 bit pattern (blocksparse_amd.quantize.quantize_test is the same in NumPy):
 *   the sign bit of x is kept in every case, a result of zero included;  a NaN stays a NaN;  +-inf and |x| >= max_float give +-max_float;
 *   otherwise ONE rounding of |x| onto the grid with step u = 2^(max(e(x), e_lo) - fbits), e(x) = the exponent field of x minus 127 (an
 *   fp32 subnormal input counts as -127):  t = |x| / u, lo = floor(t), frac = t - lo, result (lo + up) * u with
 *     mode 0  nearest, ties away from zero (the reference's default):  up = frac >= 1/2
 *     mode 1  nearest, ties to even (what the hardware formats do):    up = frac > 1/2, or frac == 1/2 and lo odd
 *     mode 2  stochastic:                                              up = r < floor(frac * 2^32), r = the element's 32 random bits
 *   a rounding that carries past max_float saturates;  without denorm a result below 2^e_lo is +-0 (a flush, not a rounding).
 * Random bits: `state` points to two uint64 on the device, {seed, offset}, the state of bsmm_ew.h.  Element i of the contiguous tensor takes
 * word i % 4 of Philox4x32-10(counter = (i / 4, 0, offset_lo, offset_hi), key = (seed_lo, seed_hi)): the result is a function of
 * (x, format, mode, seed, offset) only -- not of the grid, the access width or the storage type.  No call changes the state; a caller who
 * wants other bits from the next call advances the offset (blocksparse_amd.quantize does, as device work on the stream).
 *
 * Storage types of bsmm_quantize: fp32, and bf16 with fbits <= 7; fp16 answers BSMM_ERR_UNSUPPORTED (its exponent range cannot hold most
 * formats).  Every stored value is zero, a normal number of the storage type, or a NaN that came in.  The statistics take all three types.
 *
 * WHERE emax COMES FROM.  (1) args->emax, a host value.  (2) emax_dev non-NULL: a device int32 the kernel reads -- a
 * bsmm_quant_update_emax earlier on the same stream may have written it (no host sync), and a captured step follows it.  (3) args->group
 * = 32 (n % 32 == 0): every run of 32 consecutive elements takes e_hi = clamp(e(max finite |x| of the run) + bias_pad, nexp - 127, 127),
 * found in the same launch (four lanes of 8 elements meet by lane shuffles); non-finite elements do not enter the max, and a run with no
 * finite non-zero element uses the emax of (1) / (2).  With bias_pad = 0 this is the shared power-of-two scale of the MX formats.
 *
 * Deliberate departures from the reference:
 *   - the reference rounds twice in the subnormal range (at the value's own exponent, then onto the subnormal grid): format (4, 3, emax 8,
 *     denorm) and x = 2.484375 * 2^-9 give 3 * 2^-9 there and 2 * 2^-9 here;
 *   - a NaN does not become -max_float;
 *   - randomness is counter-based (Philox), not clock-seeded;
 *   - the exponent lives on the device (an int32), not in host memory.
 *
 * STATISTICS.  stats_out, a device float[8]: mean|x|;  stdv = sqrt(max(mean(x^2) - mean|x|^2, 0)) (the reference's quantity);  max|x|;  the
 * share with |x| >= sat_val or non-finite;  the share with x != 0 and |x| < ftz_val;  the non-finite count;  n;  0.  Non-finite elements
 * add nothing to the sums or the max; the means divide by n.  Counts are exact integers until the last conversion; sums are fp64 and go
 * through per-workgroup partials in `workspace`, added in a fixed order: the same arguments give the same bits.  Two launches: partials,
 * then one small finalize.
 */
#ifndef BSMM_QUANT_H_
#define BSMM_QUANT_H_

#include "bsmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the units of bsmm_quantize: elements a lane takes at a time, elements one workgroup covers per sweep, and the most workgroups a launch
 * has (what lies beyond BSMM_QUANT_MAX_GRID * BSMM_QUANT_WG_ELEMS is taken by a grid stride) */
#define BSMM_QUANT_LANE_ELEMS 8
#define BSMM_QUANT_WG_ELEMS 2048
#define BSMM_QUANT_MAX_GRID 2048
#define BSMM_QUANT_GROUP 32

#define BSMM_QUANT_NEAREST_AWAY 0
#define BSMM_QUANT_NEAREST_EVEN 1
#define BSMM_QUANT_STOCHASTIC 2

typedef struct bsmm_quant_args {
    int32_t ebits;      /* 1 .. 8                                                                              */
    int32_t fbits;      /* 0 .. 23; a bf16 tensor: 0 .. 7                                                      */
    int32_t emax;       /* the top exponent when emax_dev is NULL; clamped to nexp - 127 .. 127                */
    int32_t denorm;     /* 0 / 1                                                                               */
    int32_t round_mode; /* BSMM_QUANT_*                                                                        */
    int32_t group;      /* 0: one exponent per tensor;  32: one per run of 32 elements (n % 32 == 0)           */
    int32_t bias_pad;   /* added to e(M) by the group mode and by bsmm_quant_update_emax, -256 .. 256          */
    int32_t stat_mode;  /* bsmm_quant_update_emax: 0: M = max|x|;  1: M = mean + stdv_mul * stdv               */
    int32_t dtype;      /* BSMM_F32 / BSMM_F16 / BSMM_BF16                                                     */
    float   stdv_mul;
    void*   workspace; size_t workspace_bytes;   /* the statistics: >= bsmm_quant_workspace_bytes(n), 8-byte aligned */
    void*   stream;
} bsmm_quant_args;

/* Every call below answers BSMM_ERR_ARG for: args NULL, a NULL pointer that is not marked optional, n < 1 or n >= 2^31, an unknown dtype,
 * ebits / fbits / round_mode / denorm / group / bias_pad / stat_mode out of range, a bf16 tensor with fbits > 7, n % 32 != 0 with a group,
 * a state or emax_dev that is not aligned to its type, and -- the statistics -- a workspace that is too small or not 8-byte aligned. */

/* y[i] <- Q(x[i]), one launch.  y == x is allowed (in place; any other overlap is not).  state: read by round_mode 2 only, else may be
 * NULL.  emax_dev: optional.  The 16-bytes-per-lane path runs when x and y are 16-byte aligned, an element path otherwise.  fp16:
 * BSMM_ERR_UNSUPPORTED. */
int bsmm_quantize(const void* x, void* y, const uint64_t* state, const int32_t* emax_dev, int64_t n, const bsmm_quant_args* args);

/* stats_out[0 .. 8) <- the statistics of x (above).  sat_val, ftz_val >= 0 (not NaN). */
int bsmm_tensor_stats(const void* x, int64_t n, int32_t dtype, float sat_val, float ftz_val, float* stats_out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* The same statistics with sat_val = max_float and ftz_val = half the smallest grid step of the format at the CURRENT *emax_dev; stats_out
 * is optional.  The finalize launch then writes *emax_dev = clamp(e(M) + bias_pad, nexp - 127, 127) (a plain store from one lane); it stays
 * unchanged when M is 0 or no element was finite.  Reads ebits, fbits, denorm, bias_pad, stat_mode, stdv_mul, dtype, workspace, stream. */
int bsmm_quant_update_emax(const void* x, int64_t n, const bsmm_quant_args* args, int32_t* emax_dev, float* stats_out);

/* Host arithmetic only: bytes of workspace the two statistics calls need for n elements; 0 for n < 1 or n >= 2^31; non-decreasing in n. */
size_t bsmm_quant_workspace_bytes(int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* BSMM_QUANT_H_ */
