/* bsmm_ends.h -- C ABI of the two operators at the ends of a model in libbsmm_hip.so: the embedding lookup with a gradient that is summed
 * in a fixed order, and the fused softmax cross-entropy that reads the logits once and keeps `softmax - onehot` for a one-multiply backward.
 * Same boundary rules as bsmm_ew.h (bsmm.h is included for BSMM_F32 / BSMM_F16 / BSMM_BF16 and the BSMM_ERR_* codes): every pointer is a
 * device pointer owned by the caller, nothing is allocated, every call only enqueues work on `stream` (a hipStream_t) and returns; 0 = ok,
 * > 0 = a hipError_t, < 0 = BSMM_ERR_*; no environment variables, no global state, kernel choice is a function of the arguments only
 * (sizes and pointer alignment).  Arguments are checked before anything is launched.  No floating-point read-modify-write to memory: the
 * same arguments give the same bits.  Every call is safe under stream capture.
 *
 * What each entry point replaces (paths relative to the reference, openai/blocksparse):
 *   bsmm_xent_fwd / _bwd    <- ops "SoftmaxCrossEntropy" / "SoftmaxCrossEntropyGrad"   blocksparse/transformer.py:685-700,
 *                              src/transformer_op_gpu.cu:818-1009
 *   bsmm_embed_fwd / _grad  <- ops "EmbeddingLookup" / "EmbeddingLookupGrad" with sort_grad=True   blocksparse/embed.py, src/embedding_op_gpu.cu
 *
 * ---- softmax cross-entropy ------------------------------------------------------------------------------------------------------------
 * x: logits (N, K) row-major, classes contiguous, `dtype`.  labels: int32 [N].  loss: fp32 [N].  g: (N, K) `dtype`.  dy: fp32 [N].
 * dx: (N, K) `dtype`.  N >= 1, K >= 1 (no upper limit on K: the reference stops at 65536), N * K < 2^31.
 * Forward, per row, in fp32:   m = max_k x_k,   s = sum_k exp(x_k - m),   p_k = exp(x_k - m) / s,
 *     loss = log s + (m - x[label])          (not the reference's -log(max(p, 2^-24)), which clips the loss of an improbable label at 16.6)
 *     g_k  = p_k - [k == label],  rounded ONCE to the storage type; an fp16 g holds BSMM_XENT_F16_SCALE * g_k (an exact scale; |g| <= 1
 *            keeps it finite, and probabilities below 2^-14 keep their bits); bf16 and fp32 are unscaled.
 *            The label's element is computed as -(sum of the other terms) / s, not as p - 1: it keeps its bits when p is close to 1.
 * A label outside [0, K) marks an ignored row (padding): loss = 0 and every g_k = 0.
 * Non-finite logits.  x_k = -inf is a class of probability 0 (a masked class, the padding of a vocabulary): it adds nothing to s and its
 * g_k is exactly 0 on every path, wherever it lies in the row.  A label on such a class gives loss = +inf and g[label] = -1 exactly (the
 * stored value is -BSMM_XENT_F16_SCALE for fp16).  A row with no finite logit, or with a +inf or a NaN anywhere, gives a NaN loss (and g) in
 * THAT row; no other row is touched, also where several rows share a workgroup.
 * Backward:   dx_k = round(unscale(g_k) * dy[n]),   the unscale (x 2^-15 for fp16, exact) and the product in fp32.
 * Aliasing that is part of the contract: g may be the pointer x (the forward in place over the logits), and dx may be the pointer g.  Any
 * other overlap is undefined.
 * Kernel paths (bsmm_xent_path tells which one the arguments select):
 *   BSMM_XENT_SHORT     K <= BSMM_XENT_SHORT_MAX: one wave per row, four rows per workgroup, wave shuffles only, no LDS, no barrier.
 *   BSMM_XENT_REG       K <= BSMM_XENT_REG_MAX:   one workgroup of 256 lanes per row, the row stays in registers between the max, the sum
 *                       and the store: one read of x, one write of g.
 *   BSMM_XENT_REG_WIDE  K <= BSMM_XENT_WIDE_MAX:  the same with 1024 lanes.
 *   BSMM_XENT_LONG      longer rows: a running max and sum over the lanes' strips (online form), then a second sweep that re-reads the row
 *                       (from L2: it was just read) and writes g.  Never three reads.
 *   | BSMM_XENT_VEC     16 bytes per lane and access (x and g 16-byte aligned, K % 8 == 0); without it the element path, on which a
 *                       lane holds half as many elements: there the limits are BSMM_XENT_REG_MAX / 2 and BSMM_XENT_WIDE_MAX / 2.
 *   | BSMM_XENT_STRIDED more rows than the grid has room for (BSMM_XENT_MAX_GRID workgroups): a grid stride over the rows.
 * A row is never cut over workgroups: N = 3 rows of K = 65536 run on three workgroups.  Cutting one row is out of scope.
 *
 * ---- embedding lookup -----------------------------------------------------------------------------------------------------------------
 * w: (C, K) `dtype`.  idx: int32 [nIdx].  y, dy: (nIdx, K) `dtype`.  dw: fp32 (C, K) whatever the dtype.  nIdx * K < 2^31, C * K < 2^31.
 * Forward:   y[i, :] = w[idx[i], :], a copy of the bits; an index outside [0, C) gives a row of zeros.
 * Backward:  dw[c, :] = sum over {i : idx[i] == c} of dy[i, :] in fp32.  All C * K elements are stored (rows no index names get zeros),
 *            indices outside [0, C) contribute nothing.  No atomics.
 * The gradient reads its contribution rows through an inverted index the caller builds: `order`, int32 [nIdx], the permutation that sorts
 * idx ascending with ties in ascending position (a stable sort).  The sorted positions are cut into chunks of BSMM_EMBED_CHUNK rows -- a
 * constant, not a function of the grid or the device, so the bits of dw depend on (idx, dy) alone.  One team of lanes sums one chunk of one
 * column tile, whatever the distribution of the indices: a run of equal indices that lies inside a chunk is summed in position order and
 * stored; a run that crosses chunk borders leaves one fp32 partial row per chunk in `workspace`, and a second launch adds those in chunk
 * order (it also stores the zero rows).  The second launch sums the partials of one destination serially: nIdx / BSMM_EMBED_CHUNK at most.
 * An `order` that is not such a permutation gives undefined values in dw but no access outside the buffers (entries outside [0, nIdx) are
 * skipped).
 * The 16-bytes-per-lane paths need 16-byte aligned w / y (forward; rows a multiple of 16 bytes) resp. dy / dw / workspace and K % 8 == 0
 * (backward); an element path covers every other size and pointer.
 */
#ifndef BSMM_ENDS_H_
#define BSMM_ENDS_H_

#include "bsmm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSMM_XENT_F16_SCALE 32768.0f

/* bsmm_xent_path: one of the first four, OR-ed with the two flags */
#define BSMM_XENT_SHORT 1
#define BSMM_XENT_REG 2
#define BSMM_XENT_REG_WIDE 3
#define BSMM_XENT_LONG 4
#define BSMM_XENT_VEC 256
#define BSMM_XENT_STRIDED 512

#define BSMM_XENT_SHORT_MAX 1024
#define BSMM_XENT_REG_MAX 8192
#define BSMM_XENT_WIDE_MAX 32768
#define BSMM_XENT_MAX_GRID 2048

#define BSMM_EMBED_CHUNK 128

/* `which` of bsmm_ends_workspace_bytes */
#define BSMM_ENDS_XENT_FWD 0
#define BSMM_ENDS_XENT_BWD 1
#define BSMM_ENDS_EMBED_FWD 2
#define BSMM_ENDS_EMBED_GRAD 3

typedef struct bsmm_xent_args {
    const void*    x;        /* forward: logits (N, K)                                                       */
    const int32_t* labels;   /* forward: [N]                                                                 */
    float*         loss;     /* forward: [N]                                                                 */
    void*          g;        /* forward: written (may be x); backward: read                                  */
    const float*   dy;       /* backward: [N]                                                                */
    void*          dx;       /* backward: written (may be g)                                                 */
    int32_t N;               /* rows, >= 1;  N * K < 2^31                                                    */
    int32_t K;               /* classes, >= 1                                                                */
    int32_t dtype;           /* x, g, dx: BSMM_F32 / BSMM_F16 / BSMM_BF16                                    */
    int32_t reserved;        /* 0                                                                            */
    void*   stream;
} bsmm_xent_args;

typedef struct bsmm_embed_args {
    int32_t C;               /* rows of the table, >= 1;  C * K < 2^31                                       */
    int32_t K;               /* features, >= 1                                                               */
    int32_t nIdx;            /* indices, >= 1;  nIdx * K < 2^31                                              */
    int32_t dtype;           /* w, y, dy: BSMM_F32 / BSMM_F16 / BSMM_BF16                                    */
    void*   workspace; size_t workspace_bytes;   /* >= bsmm_ends_workspace_bytes(); may be NULL where that is 0 */
    void*   stream;
} bsmm_embed_args;

/* Every call below answers BSMM_ERR_ARG for: args NULL, a size < 1, a product of sizes >= 2^31, an unknown dtype, a NULL pointer the call
 * uses, labels / idx / order / loss / dy[N] / dw that are not 4-byte aligned, x / g / dx / w / y / dy(nIdx, K) that are not aligned to
 * their element, and -- bsmm_embed_grad -- a workspace that is too small or not 4-byte aligned. */

/* loss, g <- x, labels.  Reads args->x, labels, loss, g. */
int bsmm_xent_fwd(const bsmm_xent_args* args);

/* dx <- g, dy.  Reads args->g, dy, dx. */
int bsmm_xent_bwd(const bsmm_xent_args* args);

/* Host arithmetic only: the BSMM_XENT_* path bsmm_xent_fwd takes for these arguments (N, K, dtype and the alignment of x and g; the other
 * pointers are not looked at), or BSMM_ERR_ARG. */
int bsmm_xent_path(const bsmm_xent_args* args);

/* y <- w, idx.  No workspace. */
int bsmm_embed_fwd(const void* w, const int32_t* idx, void* y, const bsmm_embed_args* args);

/* dw <- dy, idx, order. */
int bsmm_embed_grad(const void* dy, const int32_t* idx, const int32_t* order, float* dw, const bsmm_embed_args* args);

/* Host arithmetic only: bytes of workspace the call `which` (BSMM_ENDS_*) needs.  Reads K and nIdx; 0 for bad arguments, for the forward
 * calls and for the cross-entropy (whose `which` values exist so that every call has one); non-decreasing in nIdx and in K. */
size_t bsmm_ends_workspace_bytes(const bsmm_embed_args* args, int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* BSMM_ENDS_H_ */
