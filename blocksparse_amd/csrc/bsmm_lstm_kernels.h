// bsmm_lstm_kernels.h -- kernels behind include/bsmm_lstm.h: the fused LSTM gates and their gradients.  Pure streaming: the forward reads 5
// tensors and writes 2, the backward reads up to 7 and writes 5; no LDS, no barriers, no workspace.  Five exponentials and five reciprocals
// per cell forward (nine each backward) against 14 bytes moved in bf16: the vector ALU is the expected bound, so the exponential and the
// reciprocal are the hardware's (__expf, v_rcp_f32) and a tanh costs one exponential.
//
// Both layouts and both forms are ONE geometry: a matrix of `rows` x `cols` whose rows are contiguous in c (and c_next, h_next, eh, ec, dc)
// and `gate_ld` (`dgate_ld`) elements apart in each of the four gate (d-gate) tensors -- axis 1: rows = N, cols = K, the bias goes by column;
// axis 0: rows = K, cols = N, gate_ld = N, the bias goes by row.  The unit of work is V consecutive elements of a row: V = 8 (4 in fp32) by
// 16-byte accesses when every pointer and every row start allows it, V = 1 otherwise (vec_load / vec_store of bsmm_vec.h; the stores pack a
// pair of bf16 by one conversion, PACK2).
//
//   lstm_cell / lstm_cell_grad   the arithmetic, once: every kernel variant calls them, the order of operations is pinned, so the same values
//                                give the same bits on every path.
//   lstm_fwd_kernel<DT, V>       grid: min(ceil(units / 256), LSTM_MAX_GRID); a lane owns one unit, the rest by a grid stride.
//   lstm_bwd_kernel<DT, V>       the same; eh or ec may be nullptr (zero).
#pragma once
#include "bsmm_vec.h"

// no contraction the source does not spell out: a product and a sum fuse only where __fmaf_rn says so
#pragma clang fp contract(off)

namespace bsmm {

constexpr int LSTM_MAX_GRID = 2048;

// 1 / (1 + exp(-x)).  x -> -inf: exp -> +inf, 1 / inf = 0;  x -> +inf: exp -> 0, 1 / 1 = 1: never inf / inf.
__device__ __forceinline__ float lstm_sigmoid(float x) { return __builtin_amdgcn_rcpf(__fadd_rn(1.f, __expf(-x))); }

// tanh through e = exp(-2 |x|) in [0, 1]: (1 - e) / (1 + e) with the sign of x; one exponential, finite for every finite x.
__device__ __forceinline__ float lstm_tanh(float x) {
    const float e = __expf(__fmul_rn(-2.f, fabsf(x)));
    return copysignf(__fmul_rn(__fsub_rn(1.f, e), __builtin_amdgcn_rcpf(__fadd_rn(1.f, e))), x);
}

// The fp32 result as it stands, before the one rounding to the storage type.  Without it the compiler folds the last multiply in front of an
// fp16 element store into the conversion (v_fma_mixlo_f16: one rounding instead of two) while the 16-byte path multiplies, then converts: the
// two paths would differ in the last bit of a few values.  Pinned inside the cell function, so that no path depends on what the compiler
// picks: that costs the 16-byte path its packed fp32 instructions (17 % more vector instructions backward) and no time -- pinning the
// element store alone measured 93.9 / 157.5 us forward / backward against 91.0 / 158.0 us (profiles/lstm_bench.md: the kernels run at the
// rate of the memory, not of the vector ALU).
__device__ __forceinline__ float lstm_pin(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

struct LstmCell {
    float si, tu, sf, so, cn, ca, h;
};

// the cell: gates i, u, f, o with their bias values (0 without a bias) and the forget bias fb
__device__ __forceinline__ LstmCell lstm_cell(float c, float i, float u, float f, float o, float bi, float bu, float bf, float bo, float fb) {
    LstmCell s;
    s.si = lstm_sigmoid(__fadd_rn(i, bi));
    s.tu = lstm_tanh(__fadd_rn(u, bu));
    s.sf = lstm_sigmoid(__fadd_rn(__fadd_rn(f, bf), fb));
    s.so = lstm_sigmoid(__fadd_rn(o, bo));
    s.cn = lstm_pin(__fmaf_rn(s.sf, c, __fmul_rn(s.si, s.tu)));
    s.ca = lstm_tanh(s.cn);
    s.h = lstm_pin(__fmul_rn(s.so, s.ca));
    return s;
}

struct LstmGrad {
    float dc, di, du, df, d_o;
};

// the gradients from the recomputed cell; 1 - t^2 as one fused multiply-add (no cancellation of a rounded square)
__device__ __forceinline__ LstmGrad lstm_cell_grad(const LstmCell& s, float c, float eh, float ec) {
    LstmGrad g;
    const float dC = __fmaf_rn(__fmul_rn(eh, s.so), __fmaf_rn(-s.ca, s.ca, 1.f), ec);
    g.di = lstm_pin(__fmul_rn(__fmul_rn(__fmul_rn(dC, s.tu), s.si), __fsub_rn(1.f, s.si)));
    g.du = lstm_pin(__fmul_rn(__fmul_rn(dC, s.si), __fmaf_rn(-s.tu, s.tu, 1.f)));
    g.df = lstm_pin(__fmul_rn(__fmul_rn(__fmul_rn(dC, c), s.sf), __fsub_rn(1.f, s.sf)));
    g.d_o = lstm_pin(__fmul_rn(__fmul_rn(__fmul_rn(eh, s.ca), s.so), __fsub_rn(1.f, s.so)));
    g.dc = lstm_pin(__fmul_rn(dC, s.sf));
    return g;
}

// the bias values of V cells: gate g of cell k at bias[g * K + k]; by row: one cell, by column: cells col .. col + V - 1 (16-byte loads when
// the bias allows it: on the wide path K and col are multiples of V).  No bias: zeros.
template <int V>
__device__ __forceinline__ void lstm_bias(const float* __restrict__ bias, uint32_t K, uint32_t row, uint32_t col, int by_row, float (&bb)[4][V]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (bias == nullptr) {
#pragma unroll
            for (int j = 0; j < V; ++j) bb[g][j] = 0.f;
        } else if (by_row) {
            const float v = bias[(size_t)g * K + row];
#pragma unroll
            for (int j = 0; j < V; ++j) bb[g][j] = v;
        } else {
            const float* p = bias + (size_t)g * K + col;
            if (V > 1 && (reinterpret_cast<uintptr_t>(bias) & 15) == 0) {
                vec_load_f32<V>(p, bb[g]);
            } else {
#pragma unroll
                for (int j = 0; j < V; ++j) bb[g][j] = p[j];
            }
        }
    }
}

// unit u -> (row, unit within the row) without an integer division: upr units per row, magic = floor(2^32 / upr) (2^32 - 1 for upr = 1).
// u * magic / 2^32 is the quotient or one below it (u / upr - u magic / 2^32 < u / 2^32 < 1), so one correction settles it.
__device__ __forceinline__ void lstm_unit(uint32_t u, uint32_t upr, uint32_t magic, uint32_t& row, uint32_t& cu) {
    row = __umulhi(u, magic);
    cu = u - row * upr;
    if (cu >= upr) {
        ++row;
        cu -= upr;
    }
}

// grid: min(ceil(units / 256), LSTM_MAX_GRID); units = rows * upr, upr = cols / V.  V > 1: every pointer 16-byte aligned, cols % V == 0,
// gate_ld % V == 0.
template <class DT, int V>
__global__ void __launch_bounds__(256) lstm_fwd_kernel(const typename DT::T* __restrict__ c, const typename DT::T* __restrict__ gi,
                                                       const typename DT::T* __restrict__ gu, const typename DT::T* __restrict__ gf,
                                                       const typename DT::T* __restrict__ go, const float* __restrict__ bias,
                                                       typename DT::T* __restrict__ cn, typename DT::T* __restrict__ hn, uint32_t cols, uint32_t upr,
                                                       uint32_t magic, uint32_t units, size_t gate_ld, uint32_t K, int by_row, float fb) {
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
        uint32_t row, cu;
        lstm_unit(u, upr, magic, row, cu);
        const uint32_t col = cu * (uint32_t)V;
        const size_t ci = (size_t)row * cols + col, gx = (size_t)row * gate_ld + col;
        float bb[4][V], vc[V], vi[V], vu[V], vf[V], vo[V], oc[V], oh[V];
        vec_load<DT, V>(c + ci, vc);
        vec_load<DT, V>(gi + gx, vi);
        vec_load<DT, V>(gu + gx, vu);
        vec_load<DT, V>(gf + gx, vf);
        vec_load<DT, V>(go + gx, vo);
        lstm_bias<V>(bias, K, row, col, by_row, bb);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const LstmCell s = lstm_cell(vc[j], vi[j], vu[j], vf[j], vo[j], bb[0][j], bb[1][j], bb[2][j], bb[3][j], fb);
            oc[j] = s.cn;
            oh[j] = s.h;
        }
        vec_store<DT, V, true>(cn + ci, oc);
        vec_store<DT, V, true>(hn + ci, oh);
    }
}

// the same grid and geometry; the d-gates dgate_ld apart.  eh / ec == nullptr: zeros (not both, the host checks).
template <class DT, int V>
__global__ void __launch_bounds__(256) lstm_bwd_kernel(const typename DT::T* __restrict__ c, const typename DT::T* __restrict__ gi,
                                                       const typename DT::T* __restrict__ gu, const typename DT::T* __restrict__ gf,
                                                       const typename DT::T* __restrict__ go, const float* __restrict__ bias,
                                                       const typename DT::T* __restrict__ eh, const typename DT::T* __restrict__ ec,
                                                       typename DT::T* __restrict__ dc, typename DT::T* __restrict__ di, typename DT::T* __restrict__ du,
                                                       typename DT::T* __restrict__ df, typename DT::T* __restrict__ d_o, uint32_t cols, uint32_t upr,
                                                       uint32_t magic, uint32_t units, size_t gate_ld, size_t dgate_ld, uint32_t K, int by_row,
                                                       float fb) {
    for (uint32_t u = blockIdx.x * 256u + threadIdx.x; u < units; u += gridDim.x * 256u) {
        uint32_t row, cu;
        lstm_unit(u, upr, magic, row, cu);
        const uint32_t col = cu * (uint32_t)V;
        const size_t ci = (size_t)row * cols + col, gx = (size_t)row * gate_ld + col, dx = (size_t)row * dgate_ld + col;
        float bb[4][V], vc[V], vi[V], vu[V], vf[V], vo[V], veh[V], vec[V];
        vec_load<DT, V>(c + ci, vc);
        vec_load<DT, V>(gi + gx, vi);
        vec_load<DT, V>(gu + gx, vu);
        vec_load<DT, V>(gf + gx, vf);
        vec_load<DT, V>(go + gx, vo);
        if (eh != nullptr) {
            vec_load<DT, V>(eh + ci, veh);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) veh[j] = 0.f;
        }
        if (ec != nullptr) {
            vec_load<DT, V>(ec + ci, vec);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) vec[j] = 0.f;
        }
        lstm_bias<V>(bias, K, row, col, by_row, bb);
        float odc[V], odi[V], odu[V], odf[V], odo[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const LstmCell s = lstm_cell(vc[j], vi[j], vu[j], vf[j], vo[j], bb[0][j], bb[1][j], bb[2][j], bb[3][j], fb);
            const LstmGrad g = lstm_cell_grad(s, vc[j], veh[j], vec[j]);
            odc[j] = g.dc;
            odi[j] = g.di;
            odu[j] = g.du;
            odf[j] = g.df;
            odo[j] = g.d_o;
        }
        vec_store<DT, V, true>(dc + ci, odc);
        vec_store<DT, V, true>(di + dx, odi);
        vec_store<DT, V, true>(du + dx, odu);
        vec_store<DT, V, true>(df + dx, odf);
        vec_store<DT, V, true>(d_o + dx, odo);
    }
}

}  // namespace bsmm
