// bsmm_sparsity_kernels.h -- kernels behind include/bsmm_sparsity.h: block norms / group-lasso decay / gate pruning of the
// [blocks][bsize][bsize] weights, and the two stages of the block-reduced full weight gradient (feature reduce, then a small
// K-contiguous GEMM whose contraction is split over workgroups and summed in a fixed order: no floating-point atomics).
//
//   stage 1  sp_reduce_a0_kernel / sp_reduce_a1_kernel: memory bound, ONE read of the activations, 16 bytes per lane and load (two loads of
//            16 bytes for fp32); out[feature block][pair][n] in a 16-bit type.
//              feature axis 0 (F, N): a lane owns 8 consecutive n and walks the bsize rows of its feature block.
//              feature axis 1 (N, F): a lane owns 8 consecutive features of one row; a block's features sit in bsize / 8 neighbouring lanes
//              (cross-lane xor reduction); a workgroup covers 64 rows x 512 features and transposes its results through LDS, so the
//              stores run along n (128 bytes per feature block and workgroup).
//   stage 2  sp_rdw_kernel: one wave per (32 x 32 output tile, slice of the contraction), v_mfma_f32_32x32x16_{bf16,f16}.  Both operands are
//            [rows][contraction] with the contraction contiguous, so both fragments are plain row loads.  K labelling (free, see
//            bsmm_common.h): in a step of 64, lane half h holds k = 32 h + 8 q + j in fragment q -- 64 contiguous bytes per lane.
//            sp_rdw_sum_kernel adds the slices in ascending order and applies scale / accumulate.
#pragma once
#include "bsmm_vec.h"

namespace bsmm {

// ---- weights: one wave per block, four blocks per workgroup ------------------------------------------------------------------
// norm_type 0: max |w|, 1: sqrt(sum w^2).  as_gate: out[b] = norm < threshold ? 0 : 1 (blocksparse_threshold_prune), else out[b] = norm.
template <class DT>
__global__ void __launch_bounds__(256) sp_block_norm_kernel(const typename DT::T* __restrict__ w, float* __restrict__ out, int blocks, int bb,
                                                            int norm_type, int as_gate, float threshold) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= blocks) return;
    const typename DT::T* p = w + (size_t)b * bb;
    float acc = 0.f;
    if (norm_type == 0) {
#pragma unroll 4
        for (int i = lane; i < bb; i += 64) acc = fmaxf(acc, fabsf(DT::to_f32(p[i])));
        acc = wave_max(acc);
    } else {
#pragma unroll 4
        for (int i = lane; i < bb; i += 64) {
            const float v = DT::to_f32(p[i]);
            acc = fmaf(v, v, acc);
        }
        acc = sqrtf(wave_sum(acc));
    }
    if (lane == 0) out[b] = as_gate ? (acc < threshold ? 0.f : 1.f) : acc;
}

// w_b -= w_b * min(rate / sqrt(sum w_b^2 + epsilon), 1); a block whose gate is exactly 0 is not touched
template <class DT>
__global__ void __launch_bounds__(256) sp_block_l2_decay_kernel(typename DT::T* __restrict__ w, const float* __restrict__ gate, int blocks, int bb,
                                                                float rate, float epsilon) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= blocks) return;
    if (gate != nullptr && gate[b] == 0.f) return;
    typename DT::T* p = w + (size_t)b * bb;
    float acc = 0.f;
#pragma unroll 4
    for (int i = lane; i < bb; i += 64) {
        const float v = DT::to_f32(p[i]);
        acc = fmaf(v, v, acc);
    }
    const float decay = fminf(rate / sqrtf(wave_sum(acc) + epsilon), 1.f);
#pragma unroll 4
    for (int i = lane; i < bb; i += 64) {
        const float v = DT::to_f32(p[i]);
        p[i] = DT::from_f32(v - v * decay);
    }
}

// gate[idx[i]] = i < keep ? 1 : 0 (idx: block ids, largest norm first); an id outside 0 .. blocks - 1 is skipped
__global__ void __launch_bounds__(256) sp_block_prune_kernel(float* __restrict__ gate, const int32_t* __restrict__ idx, int blocks, int keep) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= blocks) return;
    const uint32_t b = (uint32_t)idx[i];
    if (b < (uint32_t)blocks) gate[b] = i < keep ? 1.f : 0.f;
}

// ---- 8 consecutive elements -> 8 floats: 16-byte accesses (bsmm_vec.h) or, for a pointer that is not aligned, elements ---------------
template <class DT, bool ALIGNED>
__device__ __forceinline__ void sp_load8(const typename DT::T* p, float v[8]) {
    if constexpr (!ALIGNED) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = DT::to_f32(p[j]);
    } else {
        vec_load<DT, 8>(p, v);
    }
}

// acc <- max(acc, |v|) or acc + v^2
__device__ __forceinline__ float sp_fold(float acc, float v, int norm_type) { return norm_type == 0 ? fmaxf(acc, fabsf(v)) : fmaf(v, v, acc); }

// ---- stage 1, feature axis 0: X[p] (F, N), N % 8 == 0 -------------------------------------------------------------------------
// grid (ceil(N / 8 / 256), F / bsize, pcount)
template <class DT, class OT, bool ALIGNED>
__global__ void __launch_bounds__(256) sp_reduce_a0_kernel(PtrList8 xs, uint16_t* __restrict__ out, int N, int bsize, int pcount, int norm_type) {
    const int n = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (n >= N) return;
    const int fb = blockIdx.y, p = blockIdx.z;
    const typename DT::T* x = static_cast<const typename DT::T*>(xs.p[p]) + (size_t)fb * bsize * N + n;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int r = 0; r < bsize; ++r) {
        float v[8];
        sp_load8<DT, ALIGNED>(x + (size_t)r * N, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = sp_fold(acc[j], v[j], norm_type);
    }
    if (norm_type != 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = sqrtf(acc[j]);
    }
    uint16_t* dst = out + ((size_t)fb * pcount + p) * N + n;
    if constexpr (ALIGNED) {
        vec_store<OT, 8>(dst, acc);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[j] = OT::from_f32(acc[j]);
    }
}

// ---- stage 1, feature axis 1: X[p] (N, F) --------------------------------------------------------------------------------------
// grid (ceil(F / 512), ceil(N / 64), pcount); wave v of the workgroup takes rows 16 v .. 16 v + 15 of the 64, lane l the 8 features of chunk
// 64 * blockIdx.x + l.  vec_out: N % 8 == 0 and `out` 16-byte aligned (host decides).
constexpr int SP_A1_ROWS = 64;
template <class DT, class OT, bool ALIGNED>
__global__ void __launch_bounds__(256) sp_reduce_a1_kernel(PtrList8 xs, uint16_t* __restrict__ out, int N, int F, int bsize, int pcount, int norm_type,
                                                           int vec_out) {
    __shared__ float tile[64][SP_A1_ROWS + 1];          // [feature block of the tile][row of the tile]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = bsize >> 3;                            // lanes per feature block: 1, 2, 4, 8
    const int chunk = blockIdx.x * 64 + lane, n0 = blockIdx.y * SP_A1_ROWS, p = blockIdx.z;
    const bool live = chunk * 8 < F;
    const typename DT::T* x = static_cast<const typename DT::T*>(xs.p[p]) + (size_t)chunk * 8;
    float part[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int n = n0 + wave * 16 + i;
        float acc = 0.f;
        if (live && n < N) {
            float v[8];
            sp_load8<DT, ALIGNED>(x + (size_t)n * F, v);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = sp_fold(acc, v[j], norm_type);
        }
        part[i] = acc;
    }
    // a block's lanes are neighbours and never straddle a row or the tile (F / 8 and 64 are multiples of g)
    for (int m = 1; m < g; m <<= 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float o = __shfl_xor(part[i], m, 64);
            part[i] = norm_type == 0 ? fmaxf(part[i], o) : part[i] + o;
        }
    }
    if ((lane & (g - 1)) == 0) {
        const int bl = lane / g;
#pragma unroll
        for (int i = 0; i < 16; ++i) tile[bl][wave * 16 + i] = part[i];
    }
    __syncthreads();
    const int nb = 64 / g, FB = F / bsize;               // feature blocks of a full tile / of the tensor
    const int n = n0 + (threadIdx.x & 7) * 8;
    for (int bl = threadIdx.x >> 3; bl < nb; bl += 32) {
        const int fb = blockIdx.x * nb + bl;
        if (fb >= FB || n >= N) continue;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float t = tile[bl][(threadIdx.x & 7) * 8 + j];
            v[j] = norm_type == 0 ? t : sqrtf(t);
        }
        uint16_t* dst = out + ((size_t)fb * pcount + p) * N + n;
        if (vec_out) {                                   // (N % 8 == 0: the 8 columns are all inside)
            vec_store<OT, 8>(dst, v);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (n + j < N) dst[j] = OT::from_f32(v[j]);
        }
    }
}

// ---- stage 2 --------------------------------------------------------------------------------------------------------------------
// 8 consecutive 16-bit elements of a row, those at or beyond `lim` read as zero
template <bool ALIGNED>
__device__ __forceinline__ uint4 sp_frag8(const uint16_t* p, int lim) {
    if (lim <= 0) return zero_u4();
    if constexpr (ALIGNED) {
        if (lim >= 8) return *reinterpret_cast<const uint4*>(p);
    }
    return gather8_u16_lim(p, 1, lim);
}

// grid (tiles * S): workgroup = one wave = (tile, slice s of the contraction: k in [s * kchunk, min(Kc, (s + 1) * kchunk)), kchunk % 64 == 0).
// ws[(tile * S + s)][reg 0..15][lane 0..63]: the accumulator as it stands.
template <class DT, bool ALIGNED>
__global__ void __launch_bounds__(64) sp_rdw_kernel(const uint16_t* __restrict__ xr, const uint16_t* __restrict__ yr, float* __restrict__ ws, int CB, int KB,
                                                    int Kc, int S, int kchunk) {
    const int tile = blockIdx.x / S, s = blockIdx.x - tile * S;
    const int tn = (KB + 31) >> 5;
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int ra = (tile / tn) * 32 + r, rb = (tile % tn) * 32 + r;
    const bool va = ra < CB, vb = rb < KB;               // edge tiles: rows outside read as zero (and are never loaded)
    const uint16_t* pa = xr + (size_t)(va ? ra : 0) * Kc;
    const uint16_t* pb = yr + (size_t)(vb ? rb : 0) * Kc;
    const int k0 = s * kchunk, k1 = min(Kc, k0 + kchunk);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k = k0; k < k1; k += 64) {
        const int kk = k + 32 * h;
        uint4 a[4], b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[q] = sp_frag8<ALIGNED>(pa + kk + 8 * q, va ? k1 - (kk + 8 * q) : 0);
            b[q] = sp_frag8<ALIGNED>(pb + kk + 8 * q, vb ? k1 - (kk + 8 * q) : 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = DT::mfma32(a[q], b[q], acc);
    }
    float* dst = ws + (size_t)blockIdx.x * 1024 + lane;
#pragma unroll
    for (int i = 0; i < 16; ++i) dst[i * 64] = acc[i];
}

// dw[row][col] = scale * (sum over the slices, ascending) [+ dw[row][col]]; one thread per accumulator element
__global__ void __launch_bounds__(256) sp_rdw_sum_kernel(const float* __restrict__ ws, float* __restrict__ dw, int CB, int KB, int tiles, int S, float scale,
                                                         int accumulate) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int tile = t >> 10, e = t & 1023, reg = e >> 6, lane = e & 63;
    if (tile >= tiles) return;
    const int tn = (KB + 31) >> 5;
    const int row = (tile / tn) * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), col = (tile % tn) * 32 + (lane & 31);
    if (row >= CB || col >= KB) return;
    const float* src = ws + (size_t)tile * S * 1024 + e;
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += src[(size_t)s * 1024];
    float* d = dw + (size_t)row * KB + col;
    *d = accumulate ? fmaf(scale, sum, *d) : scale * sum;
}

}  // namespace bsmm
