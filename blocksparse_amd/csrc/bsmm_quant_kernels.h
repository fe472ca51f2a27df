// bsmm_quant_kernels.h -- kernels behind include/bsmm_quant.h: rounding onto the grid of a simulated float format and the statistics that
// choose its top exponent.  The statistics are memory bound, the rounding is bound by the vector ALU
// (profiles/quantize_bench.md).  The unit of work is a GROUP of 8 consecutive elements of the contiguous tensor, as
// in bsmm_ew_kernels.h: 16 bytes of a 16-bit type (32 of fp32, two 16-byte accesses), two Philox calls in the stochastic mode.
//
//   quant_kernel<VEC, MODE>   y = Q(x).  A lane owns group c = i / 8; the rounding is integer arithmetic on the fp32 bit pattern
//                             (quant_round), so a bf16 tensor and its fp32 upcast store equal values.  VEC: 16-byte accesses on whole groups,
//                             else element accesses.  The format's constants are derived once per lane from the spec and the exponent
//                             (a kernel argument or a device int32); in the block-scaled mode once per group from the run's largest finite
//                             magnitude: the four lanes that own a run of 32 elements meet by two lane shuffles (no LDS, no second pass).
//   quant_stats_kernel<VEC>   one 32-byte partial per workgroup: fp64 sums of |x| and x^2, the largest finite magnitude (as bits), and the
//                             counts of saturated, flushed and non-finite elements as integers.  Lanes meet in a wave reduction and LDS, in a
//                             fixed order.
//   quant_finalize_kernel     one workgroup: the partials in ascending order -> the eight statistics, and (bsmm_quant_update_emax) the new
//                             exponent, stored by one lane.
// Groups beyond the grid (at most QUANT_MAX_GRID workgroups) are taken by a grid stride.  The 16-byte accesses, the wave sum and the generator
// are those of bsmm_vec.h.
#pragma once
#include "bsmm_quant.h"
#include "bsmm_vec.h"

namespace bsmm {

constexpr int QUANT_MAX_GRID = BSMM_QUANT_MAX_GRID;
static_assert(BSMM_QUANT_LANE_ELEMS == 8 && BSMM_QUANT_WG_ELEMS == 256 * 8 && BSMM_QUANT_GROUP == 4 * 8, "the units the header exports");

// what the kernels need of bsmm_quant_args, by value
struct QuantSpec {
    int ebits, fbits, emax, denorm, round_mode, group, bias_pad, stat_mode;
    float stdv_mul;
};

// the constants of a format at one top exponent
struct QuantFmt {
    int e_lo;            // the smallest normal binade
    uint32_t max_bits;   // max_float as fp32 bits
};

__device__ __forceinline__ int quant_clamp_emax(int ebits, int emax) {
    const int nexp = ebits == 8 ? 254 : (1 << ebits) - 1;
    return emax < nexp - 127 ? nexp - 127 : (emax > 127 ? 127 : emax);
}

__device__ __forceinline__ QuantFmt quant_format(int ebits, int fbits, int denorm, int emax) {
    const int nexp = ebits == 8 ? 254 : (1 << ebits) - 1;
    const int e_hi = quant_clamp_emax(ebits, emax);
    const int sub = denorm ? fbits : 0;
    int s_min = e_hi - nexp + 1 - sub;
    s_min = s_min < -125 ? -125 : s_min;
    QuantFmt f;
    f.e_lo = s_min + sub;
    f.max_bits = ((uint32_t)(e_hi + 127) << 23) | (0x007fffffu & ~((1u << (23 - fbits)) - 1u));
    return f;
}

// Q(x) on the bit pattern; r: the element's random word (mode 2)
__device__ __forceinline__ uint32_t quant_round(uint32_t bits, const QuantFmt& f, int fbits, int denorm, int mode, uint32_t r) {
    // (no branch on the data: the special cases are selects at the end, every lane runs the same instructions)
    const uint32_t sign = bits & 0x80000000u, a = bits & 0x7fffffffu;
    const uint32_t ef = a >> 23;
    const uint32_t M = ef ? ((a & 0x007fffffu) | 0x00800000u) : a;          // |x| = M * 2^(ev - 23)
    const int e = (int)ef - 127, ev = ef ? e : -126;
    const int E = e > f.e_lo ? e : f.e_lo;
    const int sh = 23 - fbits + (E - ev);                 // t = M / 2^sh, sh >= 0
    const int shc = sh < 25 ? sh : 25;                    // (M < 2^24: every sh >= 25 gives lo = 0 and frac < 1/2)
    const uint32_t lo = M >> shc, rem = M & ((1u << shc) - 1u), twice = rem << 1, full = 1u << shc;
    // floor(frac * 2^32) = (rem << 32) >> sh without a 64-bit shift: rem < 2^sh, and rem < 2^24 makes it 0 from sh = 56 on
    const uint32_t thr = sh == 0 ? 0u : (sh <= 32 ? rem << (32 - sh) : (sh < 56 ? rem >> (sh - 32) : 0u));
    const bool up_away = twice >= full, up_even = twice > full || (twice == full && (lo & 1u)), up_rand = r < thr;
    const bool up = mode == BSMM_QUANT_NEAREST_AWAY ? up_away : (mode == BSMM_QUANT_NEAREST_EVEN ? up_even : up_rand);      // (mode: a constant in every caller)
    uint32_t q = lo + (up ? 1u : 0u);                     // the result in steps of 2^(E - fbits), <= 2^(fbits + 1)
    q = (!denorm && q < (1u << fbits)) ? 0u : q;          // below the smallest normal: flushed
    const int p = 31 - __clz((int)(q | 1u));
    uint32_t mag = ((uint32_t)(E - fbits + p + 126) << 23) + ((q << (31 - p)) >> 8);
    mag = mag > f.max_bits ? f.max_bits : mag;            // a carry past max_float saturates
    mag = q == 0u ? 0u : mag;
    mag = a >= f.max_bits ? f.max_bits : mag;             // |x| >= max_float, +-inf among them
    return a > 0x7f800000u ? bits : (sign | mag);         // a NaN stays as it came
}

// grid: min(ceil(groups / 256), QUANT_MAX_GRID), groups = ceil(total / 8).  y may be x.  VEC: x and y 16-byte aligned.
// MODE: the rounding mode as a constant, so that each kernel carries one rule for `up` (and only the stochastic one the generator).
template <class DT, bool VEC, int MODE>
__global__ void __launch_bounds__(256) quant_kernel(const typename DT::T* x, typename DT::T* y, const uint64_t* __restrict__ state,
                                                    const int32_t* __restrict__ emax_dev, QuantSpec s, uint32_t total, uint32_t groups) {
    const int emax = emax_dev != nullptr ? emax_dev[0] : s.emax;
    QuantFmt f = quant_format(s.ebits, s.fbits, s.denorm, emax);
    uint64_t seed = 0, offset = 0;
    if (MODE == BSMM_QUANT_STOCHASTIC) {
        seed = state[0];
        offset = state[1];
    }
    for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < groups; c += gridDim.x * 256u) {
        const uint32_t i0 = c * 8u;
        const int live = total - i0 < 8u ? (int)(total - i0) : 8;
        const bool whole = VEC && live == 8;
        float v[8];
        uint32_t b[8];
        if (whole) {
            vec_load<DT, 8>(x + i0, v);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = j < live ? DT::to_f32(x[i0 + j]) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = __builtin_bit_cast(uint32_t, v[j]);
        if (s.group != 0) {                               // (total % 32 == 0: the four lanes of a run are all here, with whole groups)
            uint32_t amax = 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t a = b[j] & 0x7fffffffu;
                amax = (a < 0x7f800000u && a > amax) ? a : amax;
            }
            uint32_t o = (uint32_t)__shfl_xor((int)amax, 1, 64);
            amax = o > amax ? o : amax;
            o = (uint32_t)__shfl_xor((int)amax, 2, 64);
            amax = o > amax ? o : amax;
            f = quant_format(s.ebits, s.fbits, s.denorm, amax != 0u ? (int)(amax >> 23) - 127 + s.bias_pad : emax);
        }
        uint32_t w[8];
        if (MODE == BSMM_QUANT_STOCHASTIC) {
            ew_philox(2u * c, 0u, (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w);
            ew_philox(2u * c + 1u, 0u, (uint32_t)offset, (uint32_t)(offset >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), w + 4);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) w[j] = 0u;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = __builtin_bit_cast(float, quant_round(b[j], f, s.fbits, s.denorm, MODE, w[j]));
        if (whole) {
            vec_store<DT, 8>(y + i0, v);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < live) y[i0 + j] = DT::from_f32(v[j]);
        }
    }
}

// ---- statistics ------------------------------------------------------------------------------------------------------------------------
struct QuantPartial {
    double s1, s2;                          // sums of |x| and x^2 over the finite elements
    uint32_t amax, sat, ftz, nonfinite;     // the largest finite |x| as bits; counts
};
static_assert(sizeof(QuantPartial) == 32, "bsmm_quant_workspace_bytes counts 32 bytes per workgroup");

// grid: P = min(ceil(groups / 256), QUANT_MAX_GRID) -> part[0 .. P).  from_spec: the thresholds are those of the format at emax_dev[0]
// (sat: max_float; ftz: half the smallest step), else sat_bits / ftz_bits as given.  VEC: x 16-byte aligned.
template <class DT, bool VEC>
__global__ void __launch_bounds__(256) quant_stats_kernel(const typename DT::T* __restrict__ x, uint32_t total, uint32_t groups, int from_spec,
                                                          uint32_t sat_bits, uint32_t ftz_bits, QuantSpec s, const int32_t* __restrict__ emax_dev,
                                                          QuantPartial* __restrict__ part) {
    __shared__ QuantPartial sh[4];
    if (from_spec) {
        const QuantFmt f = quant_format(s.ebits, s.fbits, s.denorm, emax_dev[0]);
        const int half_step = f.e_lo - s.fbits - 1;                       // >= -149: a power of two fp32 holds, as a subnormal below -126
        sat_bits = f.max_bits;
        ftz_bits = half_step >= -126 ? (uint32_t)(half_step + 127) << 23 : 1u << (half_step + 149);
    }
    double s1 = 0.0, s2 = 0.0;
    uint32_t amax = 0u, sat = 0u, ftz = 0u, nonf = 0u;
    for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < groups; c += gridDim.x * 256u) {
        const uint32_t i0 = c * 8u;
        const int live = total - i0 < 8u ? (int)(total - i0) : 8;
        float v[8];
        if (VEC && live == 8) {
            vec_load<DT, 8>(x + i0, v);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = j < live ? DT::to_f32(x[i0 + j]) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t a = __builtin_bit_cast(uint32_t, v[j]) & 0x7fffffffu;
            const bool finite = a < 0x7f800000u;
            const double m = finite ? (double)__builtin_bit_cast(float, a) : 0.0;
            s1 += m;
            s2 += m * m;
            amax = (finite && a > amax) ? a : amax;
            nonf += finite ? 0u : 1u;
            sat += (j < live && a >= sat_bits) || !finite ? 1u : 0u;
            ftz += (a != 0u && a < ftz_bits) ? 1u : 0u;
        }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)amax, m, 64);
        amax = o > amax ? o : amax;
        sat += (uint32_t)__shfl_xor((int)sat, m, 64);
        ftz += (uint32_t)__shfl_xor((int)ftz, m, 64);
        nonf += (uint32_t)__shfl_xor((int)nonf, m, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        QuantPartial p;
        p.s1 = s1; p.s2 = s2; p.amax = amax; p.sat = sat; p.ftz = ftz; p.nonfinite = nonf;
        sh[threadIdx.x >> 6] = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        QuantPartial p = sh[0];
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) {
            p.s1 += sh[wv].s1; p.s2 += sh[wv].s2;
            p.amax = sh[wv].amax > p.amax ? sh[wv].amax : p.amax;
            p.sat += sh[wv].sat; p.ftz += sh[wv].ftz; p.nonfinite += sh[wv].nonfinite;
        }
        part[blockIdx.x] = p;
    }
}

// grid: 1.  Lane t adds partials t, t + 256, ... in ascending order; the lanes meet in a wave reduction and LDS.  stats_out and emax_dev
// are optional.
__global__ void __launch_bounds__(256) quant_finalize_kernel(const QuantPartial* __restrict__ part, int parts, uint32_t total, float* __restrict__ stats_out,
                                                             int32_t* emax_dev, QuantSpec s) {
    __shared__ double sd[4][2];
    __shared__ unsigned long long su[4][3];
    __shared__ uint32_t sm[4];
    double s1 = 0.0, s2 = 0.0;
    unsigned long long sat = 0, ftz = 0, nonf = 0;
    uint32_t amax = 0u;
    for (int i = threadIdx.x; i < parts; i += 256) {
        const QuantPartial p = part[i];
        s1 += p.s1; s2 += p.s2;
        amax = p.amax > amax ? p.amax : amax;
        sat += p.sat; ftz += p.ftz; nonf += p.nonfinite;
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)amax, m, 64);
        amax = o > amax ? o : amax;
        sat += (unsigned long long)__shfl_xor((long long)sat, m, 64);
        ftz += (unsigned long long)__shfl_xor((long long)ftz, m, 64);
        nonf += (unsigned long long)__shfl_xor((long long)nonf, m, 64);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sd[wv][0] = s1; sd[wv][1] = s2;
        su[wv][0] = sat; su[wv][1] = ftz; su[wv][2] = nonf;
        sm[wv] = amax;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < 4; ++k) {
        s1 += sd[k][0]; s2 += sd[k][1];
        sat += su[k][0]; ftz += su[k][1]; nonf += su[k][2];
        amax = sm[k] > amax ? sm[k] : amax;
    }
    const double n = (double)total, mean = s1 / n, var = s2 / n - mean * mean, stdv = sqrt(var > 0.0 ? var : 0.0);
    const float vmax = __builtin_bit_cast(float, amax);
    if (stats_out != nullptr) {
        stats_out[0] = (float)mean;
        stats_out[1] = (float)stdv;
        stats_out[2] = vmax;
        stats_out[3] = (float)((double)sat / n);
        stats_out[4] = (float)((double)ftz / n);
        stats_out[5] = (float)nonf;
        stats_out[6] = (float)total;
        stats_out[7] = 0.f;
    }
    if (emax_dev != nullptr) {
        const float M = s.stat_mode ? (float)(mean + (double)s.stdv_mul * stdv) : vmax;
        const uint32_t mb = __builtin_bit_cast(uint32_t, M) & 0x7fffffffu;
        if (mb != 0u && mb <= 0x7f800000u && nonf < (unsigned long long)total)
            emax_dev[0] = quant_clamp_emax(s.ebits, (int)(mb >> 23) - 127 + s.bias_pad);
    }
}

}  // namespace bsmm
