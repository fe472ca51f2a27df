// bsmm_adafactor_kernels.h -- kernels behind include/bsmm_adafactor.h: Adafactor with factored second moments for a dense [C][K] tensor, a
// [K] vector and a block-sparse [blocks][bsize][bsize] tensor.  No full-size scratch: the normalised gradient x is never stored; the
// launch that sums x^2 and the launch that applies it both recompute it from grad and the NEW moments through one device function
// (adf_x2d / adf_x1d), so both see the same bits.  No atomics: every partial sum has a workspace slot of its own, every slot a call
// reads that call has stored, and partials are added in a fixed order.
//
//   2-d form, 4 launches over tiles of ADF_SLAB rows x (256 V) columns (V = 4 on the 16-byte path, 1 on the element path; a lane owns V
//   consecutive columns of the tile, a workgroup walks tiles w, w + G, ...):
//     adf2_partial    per tile: column partials (a lane's chain over the slab's rows) -> colpart[slab][k]; row partials (the lane's V
//                     values, wave_sum, the four waves in order) -> rowpart[row][chunk]
//     adf2_finalize   cv_k: wave w of a workgroup adds slabs w, w + 4, ... of 64 columns, the four waves are added in order;
//                     rv_c: one wave per row, lane l adds chunks l, l + 64, ..., wave_sum; the new rv of a wave's rows are added in a
//                     chain, the four waves in order -> rvslots[workgroup]
//     adf2_x2         m = (fixed-order sum of rvslots) / C; a lane adds the V x^2 of a row, the rows of a tile, its tiles; the workgroup's
//                     256 lanes by wave_sum and the four waves in order -> x2slots[workgroup]
//     adf2_apply      rate from the fixed-order sum of x2slots; p -= rate x, the 16-bit copy
//   1-d form, 2 launches: adf1_moment (cv, x^2 partials -> x2slots), adf1_apply.
//   block form, 2 launches, one wave per block (4 per workgroup, blocks w, w + 4 G, ...):
//     adfb_moment     the block is read once into registers (bsize 32: 16 values per lane, 64: 64); a row lies in bsize / V neighbouring
//                     lanes, row sums are an xor tree over those lanes, column sums a lane's chain over its steps and an xor tree over
//                     the lanes that hold the same columns; new rv, cv and the block's m = mean rv are stored, the block's x^2 are summed
//                     (lane chain, wave_sum) and added to the wave's chain over its blocks; the four waves in order -> x2slots[workgroup],
//                     the live-block count (integers) -> liveslots[workgroup]
//     adfb_apply      rate from the sums of both slot arrays; p -= rate x for the live blocks
//
// Chain lengths.  A "chain" is a run of fp32 additions into one accumulator; its terms may be partial sums.  ADF_CHAIN = 64 bounds every
// chain while rows <= 8192 (column slabs per wave), cols <= 4 Mi (row chunks per lane), rows <= 64 Ki (rv sums), tiles <= 64 * 2048
// (x^2: a tile adds ADF_SLAB terms, then one term per tile) and blocks <= 256 Ki; beyond those sizes the strided chains grow in proportion
// (ceil(size / limit) * 64), nothing else changes.
#pragma once
#include "bsmm_optim_kernels.h"

namespace bsmm {

constexpr int ADF_THREADS = 256;
constexpr int ADF_SLAB = 32;             // rows of a tile
constexpr int ADF_CHAIN = 64;            // see above
constexpr int ADF_X2_SLOTS = 2048;       // x^2 partials of the dense forms (= workgroups at most)
constexpr int ADF_RV_SLOTS = 256;        // partial sums of the new rv
constexpr int ADF_BLK_SLOTS = 1024;      // block form: x^2 partials, then as many live counts
constexpr int ADF_COL_GRID = 1024;       // workgroups of adf2_finalize that own columns
constexpr int ADF_HEAD = ADF_X2_SLOTS + ADF_RV_SLOTS;      // floats in front of the per-shape sections of the workspace

struct AdfParams {
    float lr, decay, omd, epsilon, clip_thresh, grad_scale, saturate;      // omd = 1 - decay in fp32
    int zero_infs, zero_nans;
};

// ---- the arithmetic, one copy -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float adf_grad(float g, const AdfParams& a, float gs) { return opt_pre(g, a.zero_infs, a.zero_nans, a.saturate) * gs; }
__device__ __forceinline__ float adf_sq(float g, const AdfParams& a) { return fmaf(g, g, a.epsilon); }
__device__ __forceinline__ float adf_moment(float old, float mean, const AdfParams& a) { return fmaf(a.decay, old, a.omd * mean); }
__device__ __forceinline__ float adf_rsqrt(float v) { return 1.f / sqrtf(v); }                    // IEEE square root, IEEE division
__device__ __forceinline__ float adf_x2d(float g, float row_factor, float col_factor) { return g * (row_factor * col_factor); }
__device__ __forceinline__ float adf_x1d(float g, float cv) { return g / sqrtf(cv); }
__device__ __forceinline__ float adf_rate(float sum_x2, float inv_n, const AdfParams& a) {
    return a.lr / fmaxf(sqrtf(sum_x2 * inv_n) / a.clip_thresh, 1.f);
}

// x0^2 + x1^2 + ... of a lane's V values, left to right
template <int V>
__device__ __forceinline__ float adf_sum_sq(const float* x) {
    float q = x[0] * x[0];
#pragma unroll
    for (int j = 1; j < V; ++j) q = fmaf(x[j], x[j], q);
    return q;
}

// n slots in a fixed order: lane t adds slots t, t + 256, ..., then the workgroup's sum; every thread gets the same bits
__device__ __forceinline__ float adf_slot_sum(const float* __restrict__ slots, int n, float* share) {
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += ADF_THREADS) acc += slots[i];
    const float total = opt_group_sum(acc, share);
    __syncthreads();                                         // share is free again
    return total;
}

template <class PT16, int V>
__device__ __forceinline__ void adf_store16(void* param16, size_t off, const float* p) {
    vec_store<PT16, V>(static_cast<typename PT16::T*>(param16) + off, p);
}

// the 16-bit working copy: p16 = 0 (none) / BSMM_F16 / BSMM_BF16, uniform over the launch
template <int V>
__device__ __forceinline__ void adf_store_copy(void* param16, int p16, size_t off, const float* p) {
    if (p16 == BSMM_F16) adf_store16<DTf16, V>(param16, off, p);
    else if (p16 == BSMM_BF16) adf_store16<DTbf16, V>(param16, off, p);
}

// ---- 2-d form ---------------------------------------------------------------------------------------------------------------------------
struct AdfTile {
    size_t slab, chunk, row0, col;
    int nrows;
    bool on;                                                 // this lane's columns exist (16-byte path: cols % 4 == 0, all four or none)
};

template <int V>
__device__ __forceinline__ AdfTile adf_tile(size_t t, size_t nchunks, size_t C, size_t K) {
    AdfTile x;
    x.slab = t / nchunks;
    x.chunk = t - x.slab * nchunks;
    x.row0 = x.slab * ADF_SLAB;
    x.col = x.chunk * (size_t)(ADF_THREADS * V) + (size_t)threadIdx.x * V;
    const size_t left = C - x.row0;
    x.nrows = left < (size_t)ADF_SLAB ? (int)left : ADF_SLAB;
    x.on = x.col < K;
    return x;
}

template <class GT, bool VEC>
__global__ void __launch_bounds__(ADF_THREADS) adf2_partial_kernel(const typename GT::T* __restrict__ grad, const float* __restrict__ norm_scale,
                                                                   float* __restrict__ colpart, float* __restrict__ rowpart, size_t C, size_t K,
                                                                   size_t Kpad, size_t nchunks, size_t ntiles, AdfParams a) {
    constexpr int V = VEC ? 4 : 1;
    __shared__ float rowshare[ADF_SLAB][4];
    const float ns = norm_scale != nullptr ? *norm_scale : 1.f;
    if (ns == 0.f) return;                                   // the clip's "skip this step"
    const float gs = a.grad_scale * ns;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const AdfTile tl = adf_tile<V>(t, nchunks, C, K);
        float cacc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) cacc[j] = 0.f;
        for (int r0 = 0; r0 < tl.nrows; r0 += 4) {           // four rows' loads in flight, then their sums in row order
            float g[4][V];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (tl.on && r0 + u < tl.nrows) vec_load<GT, V>(grad + (tl.row0 + r0 + u) * K + tl.col, g[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (r0 + u >= tl.nrows) break;
                float q = 0.f;
                if (tl.on) {
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const float s = adf_sq(adf_grad(g[u][j], a, gs), a);
                        cacc[j] += s;
                        q = j == 0 ? s : q + s;
                    }
                }
                q = wave_sum(q);
                if (lane == 0) rowshare[r0 + u][wave] = q;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < tl.nrows) {
            const float* w = rowshare[threadIdx.x];
            rowpart[(tl.row0 + threadIdx.x) * nchunks + tl.chunk] = ((w[0] + w[1]) + w[2]) + w[3];
        }
        if (tl.on) vec_store_f32<V>(colpart + tl.slab * Kpad + tl.col, cacc);
        __syncthreads();                                     // rowshare is free again
    }
}

template <int UNUSED = 0>
__global__ void __launch_bounds__(ADF_THREADS) adf2_finalize_kernel(float* __restrict__ cv, float* __restrict__ rv, const float* __restrict__ norm_scale,
                                                                    const float* __restrict__ colpart, const float* __restrict__ rowpart,
                                                                    float* __restrict__ rvslots, size_t C, size_t K, size_t Kpad, size_t nslabs,
                                                                    size_t nchunks, int ncolwg, int nrvwg, float inv_c, float inv_k, AdfParams a) {
    __shared__ float share[4][64];
    const float ns = norm_scale != nullptr ? *norm_scale : 1.f;
    if (ns == 0.f) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)blockIdx.x < ncolwg) {
        const size_t ngroups = (K + 63) / 64;
        for (size_t gi = blockIdx.x; gi < ngroups; gi += (size_t)ncolwg) {
            const size_t k = gi * 64 + lane;
            float acc = 0.f;
            if (k < K)
                for (size_t s = wave; s < nslabs; s += 4) acc += colpart[s * Kpad + k];
            share[wave][lane] = acc;
            __syncthreads();
            if (wave == 0 && k < K) {
                const float sum = ((share[0][lane] + share[1][lane]) + share[2][lane]) + share[3][lane];
                cv[k] = adf_moment(cv[k], sum * inv_c, a);
            }
            __syncthreads();
        }
    } else {
        const size_t w0 = (size_t)((int)blockIdx.x - ncolwg) * 4 + wave, nw = (size_t)nrvwg * 4;
        float racc = 0.f;
        for (size_t row = w0; row < C; row += nw) {
            float acc = 0.f;
            for (size_t c = lane; c < nchunks; c += 64) acc += rowpart[row * nchunks + c];
            acc = wave_sum(acc);
            const float nv = adf_moment(rv[row], acc * inv_k, a);
            if (lane == 0) rv[row] = nv;
            racc += nv;
        }
        if (lane == 0) share[0][wave] = racc;
        __syncthreads();
        if (threadIdx.x == 0) rvslots[(int)blockIdx.x - ncolwg] = ((share[0][0] + share[0][1]) + share[0][2]) + share[0][3];
    }
}

// the row factors of a slab, 1 / sqrt(rv_c / m), once per tile
__device__ __forceinline__ void adf_row_factors(float* arow, const float* __restrict__ rv, const AdfTile& tl, float m) {
    if ((int)threadIdx.x < tl.nrows) arow[threadIdx.x] = adf_rsqrt(rv[tl.row0 + threadIdx.x] / m);
    __syncthreads();
}

template <class GT, bool VEC>
__global__ void __launch_bounds__(ADF_THREADS) adf2_x2_kernel(const typename GT::T* __restrict__ grad, const float* __restrict__ norm_scale,
                                                              const float* __restrict__ cv, const float* __restrict__ rv,
                                                              const float* __restrict__ rvslots, float* __restrict__ x2slots, size_t C, size_t K,
                                                              size_t nchunks, size_t ntiles, int nrvwg, float inv_c, AdfParams a) {
    constexpr int V = VEC ? 4 : 1;
    __shared__ float share[4];
    __shared__ float arow[ADF_SLAB];
    const float ns = norm_scale != nullptr ? *norm_scale : 1.f;
    if (ns == 0.f) return;
    const float gs = a.grad_scale * ns;
    const float m = adf_slot_sum(rvslots, nrvwg, share) * inv_c;
    float acc = 0.f;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const AdfTile tl = adf_tile<V>(t, nchunks, C, K);
        adf_row_factors(arow, rv, tl, m);
        if (tl.on) {
            float b[V];
            vec_load_f32<V>(cv + tl.col, b);
#pragma unroll
            for (int j = 0; j < V; ++j) b[j] = adf_rsqrt(b[j]);
            float tacc = 0.f;
#pragma unroll 4
            for (int r = 0; r < tl.nrows; ++r) {
                float x[V];
                vec_load<GT, V>(grad + (tl.row0 + r) * K + tl.col, x);
#pragma unroll
                for (int j = 0; j < V; ++j) x[j] = adf_x2d(adf_grad(x[j], a, gs), arow[r], b[j]);
                tacc += adf_sum_sq<V>(x);
            }
            acc += tacc;
        }
        __syncthreads();                                     // arow is free again
    }
    const float total = opt_group_sum(acc, share);
    if (threadIdx.x == 0) x2slots[blockIdx.x] = total;
}

template <class GT, bool VEC>
__global__ void __launch_bounds__(ADF_THREADS) adf2_apply_kernel(float* __restrict__ param, void* __restrict__ param16, int p16,
                                                                 const typename GT::T* __restrict__ grad, const float* __restrict__ norm_scale,
                                                                 const float* __restrict__ cv, const float* __restrict__ rv,
                                                                 const float* __restrict__ rvslots, const float* __restrict__ x2slots, size_t C,
                                                                 size_t K, size_t nchunks, size_t ntiles, int nrvwg, int nx2, float inv_c, float inv_n,
                                                                 AdfParams a) {
    constexpr int V = VEC ? 4 : 1;
    __shared__ float share[4];
    __shared__ float arow[ADF_SLAB];
    const float ns = norm_scale != nullptr ? *norm_scale : 1.f;
    if (ns == 0.f) return;
    const float gs = a.grad_scale * ns;
    const float m = adf_slot_sum(rvslots, nrvwg, share) * inv_c;
    const float rate = adf_rate(adf_slot_sum(x2slots, nx2, share), inv_n, a);
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const AdfTile tl = adf_tile<V>(t, nchunks, C, K);
        adf_row_factors(arow, rv, tl, m);
        if (tl.on) {
            float b[V];
            vec_load_f32<V>(cv + tl.col, b);
#pragma unroll
            for (int j = 0; j < V; ++j) b[j] = adf_rsqrt(b[j]);
#pragma unroll 4
            for (int r = 0; r < tl.nrows; ++r) {
                const size_t off = (tl.row0 + r) * K + tl.col;
                float x[V], p[V];
                vec_load<GT, V>(grad + off, x);
                vec_load_f32<V>(param + off, p);
#pragma unroll
                for (int j = 0; j < V; ++j) p[j] = fmaf(-rate, adf_x2d(adf_grad(x[j], a, gs), arow[r], b[j]), p[j]);
                vec_store_f32<V>(param + off, p);
                adf_store_copy<V>(param16, p16, off, p);
            }
        }
        __syncthreads();
    }
}

// ---- 1-d form ---------------------------------------------------------------------------------------------------------------------------
template <class GT, bool VEC>
__global__ void __launch_bounds__(ADF_THREADS) adf1_moment_kernel(const typename GT::T* __restrict__ grad, const float* __restrict__ norm_scale,
                                                                  float* __restrict__ cv, float* __restrict__ x2slots, size_t K, AdfParams a) {
    constexpr int V = VEC ? 4 : 1;
    __shared__ float share[4];
    const float ns = norm_scale != nullptr ? *norm_scale : 1.f;
    if (ns == 0.f) return;
    const float gs = a.grad_scale * ns;
    const size_t units = K / V, nthreads = (size_t)gridDim.x * ADF_THREADS;
    float acc = 0.f;
    for (size_t u = (size_t)blockIdx.x * ADF_THREADS + threadIdx.x; u < units; u += nthreads) {
        float x[V], v[V];
        vec_load<GT, V>(grad + u * V, x);
        vec_load_f32<V>(cv + u * V, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float g = adf_grad(x[j], a, gs);
            v[j] = adf_moment(v[j], adf_sq(g, a), a);
            x[j] = adf_x1d(g, v[j]);
        }
        vec_store_f32<V>(cv + u * V, v);
        acc += adf_sum_sq<V>(x);
    }
    const float total = opt_group_sum(acc, share);
    if (threadIdx.x == 0) x2slots[blockIdx.x] = total;
}

template <class GT, bool VEC>
__global__ void __launch_bounds__(ADF_THREADS) adf1_apply_kernel(float* __restrict__ param, void* __restrict__ param16, int p16,
                                                                 const typename GT::T* __restrict__ grad, const float* __restrict__ norm_scale,
                                                                 const float* __restrict__ cv, const float* __restrict__ x2slots, size_t K, int nx2,
                                                                 float inv_n, AdfParams a) {
    constexpr int V = VEC ? 4 : 1;
    __shared__ float share[4];
    const float ns = norm_scale != nullptr ? *norm_scale : 1.f;
    if (ns == 0.f) return;
    const float gs = a.grad_scale * ns;
    const float rate = adf_rate(adf_slot_sum(x2slots, nx2, share), inv_n, a);
    const size_t units = K / V, nthreads = (size_t)gridDim.x * ADF_THREADS;
    for (size_t u = (size_t)blockIdx.x * ADF_THREADS + threadIdx.x; u < units; u += nthreads) {
        float x[V], v[V], p[V];
        vec_load<GT, V>(grad + u * V, x);
        vec_load_f32<V>(cv + u * V, v);
        vec_load_f32<V>(param + u * V, p);
#pragma unroll
        for (int j = 0; j < V; ++j) p[j] = fmaf(-rate, adf_x1d(adf_grad(x[j], a, gs), v[j]), p[j]);
        vec_store_f32<V>(param + u * V, p);
        adf_store_copy<V>(param16, p16, u * V, p);
    }
}

// ---- block form -------------------------------------------------------------------------------------------------------------------------
// How a wave holds a bsize x bsize block, V consecutive elements per lane and step.
template <int BS, int V>
struct AdfBlockMap {
    static constexpr int BB = BS * BS;
    static constexpr int LPR = BS / V;                                   // lanes that share a row
    static constexpr int ACTIVE = BB / V < 64 ? BB / V : 64;             // lanes with elements (bsize 8 on the 16-byte path: 16)
    static constexpr int STEPS = BB / (ACTIVE * V);
    static constexpr int RPS = ACTIVE / LPR;                             // rows per step
};

__device__ __forceinline__ int adf_wave_sum_int(int v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <class GT, int BS, bool VEC>
__global__ void __launch_bounds__(ADF_THREADS) adfb_moment_kernel(const typename GT::T* __restrict__ grad, const float* __restrict__ norm_scale,
                                                                  const float* __restrict__ gate, float* __restrict__ cv, float* __restrict__ rv,
                                                                  float* __restrict__ mblk, float* __restrict__ x2slots, int* __restrict__ liveslots,
                                                                  size_t blocks, AdfParams a) {
    constexpr int V = VEC ? 4 : 1;
    using M = AdfBlockMap<BS, V>;
    constexpr float INV = 1.f / BS;
    __shared__ float share[4];
    __shared__ int ishare[4];
    const float ns = norm_scale != nullptr ? *norm_scale : 1.f;
    if (ns == 0.f) return;
    const float gs = a.grad_scale * ns;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool act = lane < M::ACTIVE;
    const int rl = lane / M::LPR, cl = (lane % M::LPR) * V;  // row inside a step, first column
    float xacc = 0.f;
    int live = 0;
    for (size_t b = (size_t)blockIdx.x * 4 + wave; b < blocks; b += (size_t)gridDim.x * 4) {
        if (gate != nullptr && gate[b] == 0.f) continue;     // uniform over the wave: the block is neither read nor written
        ++live;
        const typename GT::T* gb = grad + b * M::BB;
        float* rvb = rv + b * BS;
        float* cvb = cv + b * BS;
        float g[M::STEPS][V], rnew[M::STEPS], cacc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) cacc[j] = 0.f;
        float racc = 0.f;
#pragma unroll
        for (int i = 0; i < M::STEPS; ++i) {
            float q = 0.f;
            if (act) {
                vec_load<GT, V>(gb + i * (M::ACTIVE * V) + lane * V, g[i]);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    g[i][j] = adf_grad(g[i][j], a, gs);
                    const float s = adf_sq(g[i][j], a);
                    cacc[j] += s;
                    q = j == 0 ? s : q + s;
                }
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) g[i][j] = 0.f;
            }
#pragma unroll
            for (int m = M::LPR / 2; m > 0; m >>= 1) q += __shfl_xor(q, m, 64);      // the row's sum, in every lane of the row
            rnew[i] = adf_moment(act ? rvb[i * M::RPS + rl] : 0.f, q * INV, a);
            racc += rnew[i];
        }
#pragma unroll
        for (int m = M::LPR; m < M::ACTIVE; m <<= 1) {       // across the lanes that hold other rows: column sums, the sum of the new rv
#pragma unroll
            for (int j = 0; j < V; ++j) cacc[j] += __shfl_xor(cacc[j], m, 64);
            racc += __shfl_xor(racc, m, 64);
        }
        const float mb = racc * INV;
        float bcol[V];
        if (act) {
            vec_load_f32<V>(cvb + cl, bcol);
#pragma unroll
            for (int j = 0; j < V; ++j) bcol[j] = adf_moment(bcol[j], cacc[j] * INV, a);
            if (rl == 0) vec_store_f32<V>(cvb + cl, bcol);
            if (cl == 0) {
#pragma unroll
                for (int i = 0; i < M::STEPS; ++i) rvb[i * M::RPS + rl] = rnew[i];
            }
#pragma unroll
            for (int j = 0; j < V; ++j) bcol[j] = adf_rsqrt(bcol[j]);
        }
        if (lane == 0) mblk[b] = mb;
        float bacc = 0.f;
        if (act) {
#pragma unroll
            for (int i = 0; i < M::STEPS; ++i) {
                const float arow = adf_rsqrt(rnew[i] / mb);
                float x[V];
#pragma unroll
                for (int j = 0; j < V; ++j) x[j] = adf_x2d(g[i][j], arow, bcol[j]);
                bacc += adf_sum_sq<V>(x);
            }
        }
        xacc += wave_sum(bacc);
    }
    if (lane == 0) {
        share[wave] = xacc;
        ishare[wave] = live;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        x2slots[blockIdx.x] = ((share[0] + share[1]) + share[2]) + share[3];
        liveslots[blockIdx.x] = ishare[0] + ishare[1] + ishare[2] + ishare[3];
    }
}

template <class GT, bool VEC>
__global__ void __launch_bounds__(ADF_THREADS) adfb_apply_kernel(float* __restrict__ param, void* __restrict__ param16, int p16,
                                                                 const typename GT::T* __restrict__ grad, const float* __restrict__ norm_scale,
                                                                 const float* __restrict__ gate, const float* __restrict__ cv,
                                                                 const float* __restrict__ rv, const float* __restrict__ mblk,
                                                                 const float* __restrict__ x2slots, const int* __restrict__ liveslots, int nslots,
                                                                 size_t blocks, int bs, AdfParams a) {
    constexpr int V = VEC ? 4 : 1;
    __shared__ float share[4];
    __shared__ int ishare[4];
    const float ns = norm_scale != nullptr ? *norm_scale : 1.f;
    if (ns == 0.f) return;
    const float gs = a.grad_scale * ns;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float total = adf_slot_sum(x2slots, nslots, share);
    int live = 0;
    for (int i = threadIdx.x; i < nslots; i += ADF_THREADS) live += liveslots[i];
    live = adf_wave_sum_int(live);
    if (lane == 0) ishare[wave] = live;
    __syncthreads();
    live = ishare[0] + ishare[1] + ishare[2] + ishare[3];
    if (live == 0) return;                                   // every gate is 0: nothing is stored
    const int bb = bs * bs;
    const float rate = adf_rate(total, 1.f / ((float)live * (float)bb), a);
    const int lpr = bs / V, active = bb / V < 64 ? bb / V : 64, steps = bb / (active * V), rps = active / lpr;
    const int rl = lane / lpr, cl = (lane % lpr) * V;
    if (lane >= active) return;
    for (size_t b = (size_t)blockIdx.x * 4 + wave; b < blocks; b += (size_t)gridDim.x * 4) {
        if (gate != nullptr && gate[b] == 0.f) continue;
        const float mb = mblk[b];
        float bcol[V];
        vec_load_f32<V>(cv + b * bs + cl, bcol);
#pragma unroll
        for (int j = 0; j < V; ++j) bcol[j] = adf_rsqrt(bcol[j]);
#pragma unroll 4
        for (int i = 0; i < steps; ++i) {
            const float arow = adf_rsqrt(rv[b * bs + i * rps + rl] / mb);
            const size_t off = b * bb + (size_t)(i * active + lane) * V;
            float x[V], p[V];
            vec_load<GT, V>(grad + off, x);
            vec_load_f32<V>(param + off, p);
#pragma unroll
            for (int j = 0; j < V; ++j) p[j] = fmaf(-rate, adf_x2d(adf_grad(x[j], a, gs), arow, bcol[j]), p[j]);
            vec_store_f32<V>(param + off, p);
            adf_store_copy<V>(param16, p16, off, p);
        }
    }
}

}  // namespace bsmm
