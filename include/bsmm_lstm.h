/* bsmm_lstm.h -- C ABI of the fused LSTM gates in libbsmm_hip.so: the cell update between two block-sparse matmuls of a recurrent model and
 * its gradients, in BOTH activation layouts of the matmul, for the fused gate tensor a layer norm with segments = 4 produces and for four
 * separate gate tensors.  Same boundary rules as bsmm_ew.h (bsmm.h is included for BSMM_F32 / BSMM_F16 / BSMM_BF16 and the BSMM_ERR_*
 * codes): every pointer is a device pointer owned by the caller, nothing is allocated, every call only enqueues work on `stream` (a
 * hipStream_t) and returns; 0 = ok, > 0 = a hipError_t, < 0 = BSMM_ERR_*; no environment variables, no global state, kernel choice is a
 * function of the arguments only (sizes and pointer alignment).  Arguments are checked before anything is launched.
 *
 * What the entry points replace (paths relative to the reference, openai/blocksparse):
 *   bsmm_lstm_gates / _grad   <- ops "LSTMGates" / "LSTMGates4" and their gradients   blocksparse/lstm.py:22-74, src/lstm_op.cc,
 *                                src/lstm_op_gpu.cu; the axis-0 form has no counterpart there.
 *
 * Shapes: K cells, N = product of all other dims, K * N < 2^31.
 *   axis 1: c, c_next, h_next, eh, ec, dc are (N, K) row-major.  A gate tensor is (N, K) with `gate_ld` elements between its rows: four
 *           separate tensors (gate_ld = K) or the column slices i | u | f | o of ONE (N, 4K) tensor (gate_ld = 4K, the pointers K elements
 *           apart).  The four d-gate outputs likewise with `dgate_ld`.
 *   axis 0: c and the others are (K, N) row-major; every gate tensor is a contiguous (K, N): four separate tensors or the four chunks of ONE
 *           (4K, N) tensor.  gate_ld and dgate_ld are ignored.
 * bias: fp32 [4K] in gate order i, u, f, o, or NULL; indexed by column on axis 1 and by row on axis 0.
 *
 * Element-wise, in fp32, one rounding to the storage type per stored value (fb = forget_bias):
 *   si = sigmoid(i + b_i)    tu = tanh(u + b_u)    sf = sigmoid(f + b_f + fb)    so = sigmoid(o + b_o)
 *   c_next = sf * c + si * tu        ca = tanh(c_next)  (of the fp32 c_next, not of the stored one)        h_next = so * ca
 * Backward (eh, ec: the gradients of h_next and c_next; either may be NULL and counts as zero, not both); the activations are recomputed
 * from the inputs:
 *   dC = eh * so * (1 - ca^2) + ec
 *   di = dC * tu * si * (1 - si)    du = dC * si * (1 - tu^2)    df = dC * c * sf * (1 - sf)    do = eh * ca * so * (1 - so)    dc = dC * sf
 * sigmoid and tanh are finite and take their limits for every finite input.  Every kernel calls one cell function with a pinned order of
 * operations: the same values give the same bits whatever the axis, the form and the path.
 *
 * The gradient of the bias is bsmm_bias_act_grad (bsmm_ew.h) with act 0 on the stored d-gates (K' = 4K on the fused tensor).
 *
 * The 16-bytes-per-lane path runs when every pointer is 16-byte aligned and so is every row start -- K, gate_ld (dgate_ld) multiples of 8
 * (4 in fp32) on axis 1, N such a multiple on axis 0 -- an element path covers every other size and pointer.
 */
#ifndef BSMM_LSTM_H_
#define BSMM_LSTM_H_

#include "bsmm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bsmm_lstm_args {
    int32_t K;            /* cells;  4 * K must fit an int32                                                  */
    int32_t N;            /* product of all other dims, >= 1;  K * N < 2^31                                   */
    int32_t axis;         /* 0: c is (K, N) row-major;  1: c is (N, K) row-major                              */
    int32_t dtype;        /* c, gates, c_next, h_next, eh, ec, dc, d-gates: BSMM_F32 / BSMM_F16 / BSMM_BF16   */
    int64_t gate_ld;      /* axis 1: elements between rows of a gate tensor, >= K;  axis 0: ignored           */
    int64_t dgate_ld;     /* the same for the four d-gate outputs (read by bsmm_lstm_gates_grad only)         */
    float   forget_bias;
    void*   stream;
} bsmm_lstm_args;

/* Both calls answer BSMM_ERR_ARG for: args NULL, K / N < 1, K * N >= 2^31, 4 * K >= 2^31, axis not 0 / 1, an unknown dtype, a NULL pointer
 * that is not marked optional, and on axis 1 a gate_ld (the gradient: or a dgate_ld) below K. */

/* c_next, h_next <- c, the four gates [, bias] */
int bsmm_lstm_gates(const void* c, const void* i, const void* u, const void* f, const void* o, const float* bias /* [4K] or NULL */,
                    void* c_next, void* h_next, const bsmm_lstm_args* args);

/* dc, di, du, df, d_o <- c, the four gates [, bias], eh and / or ec.  BSMM_ERR_ARG when eh and ec are both NULL. */
int bsmm_lstm_gates_grad(const void* c, const void* i, const void* u, const void* f, const void* o, const float* bias,
                         const void* eh /* or NULL */, const void* ec /* or NULL */,
                         void* dc, void* di, void* du, void* df, void* d_o, const bsmm_lstm_args* args);

#ifdef __cplusplus
}
#endif
#endif /* BSMM_LSTM_H_ */
