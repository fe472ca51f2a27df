// bsmm_quant.hip -- C-ABI entry points of include/bsmm_quant.h: argument checks, the cut of the work over workgroups (a function of n
// only), then launches of the kernels in bsmm_quant_kernels.h.  No allocation, no host sync, no environment, no state.
#include <cstdint>

#include "bsmm_quant.h"
#include "bsmm_quant_kernels.h"
#include "bsmm_host.h"

using namespace bsmm;

namespace {

inline bool n_ok(int64_t n) { return n >= 1 && n < ((int64_t)1 << 31); }
inline uint32_t groups_of(int64_t n) { return (uint32_t)((n + 7) / 8); }
inline unsigned grid_of(int64_t n) { return capped((groups_of(n) + 255u) / 256u, QUANT_MAX_GRID); }

// the fields every call reads
int check_spec(const bsmm_quant_args* a) {
    if (a == nullptr || !dtype_ok(a->dtype)) return BSMM_ERR_ARG;
    if (a->ebits < 1 || a->ebits > 8 || a->fbits < 0 || a->fbits > 23 || (a->denorm != 0 && a->denorm != 1)) return BSMM_ERR_ARG;
    if (a->bias_pad < -256 || a->bias_pad > 256) return BSMM_ERR_ARG;
    return BSMM_OK;
}

int check_workspace(const void* ws, size_t bytes, int64_t n) {
    if (ws == nullptr || !aligned_to(ws, 8) || bytes < (size_t)grid_of(n) * sizeof(QuantPartial)) return BSMM_ERR_ARG;
    return BSMM_OK;
}

QuantSpec spec_of(const bsmm_quant_args* a) {
    QuantSpec s;
    s.ebits = a->ebits; s.fbits = a->fbits; s.emax = a->emax; s.denorm = a->denorm; s.round_mode = a->round_mode; s.group = a->group;
    s.bias_pad = a->bias_pad; s.stat_mode = a->stat_mode; s.stdv_mul = a->stdv_mul;
    return s;
}

// partials, then the finalize; from_spec: the thresholds of the format at *emax_dev, and the finalize writes *emax_dev
int stats(const void* x, int64_t n, int dtype, int from_spec, uint32_t sat_bits, uint32_t ftz_bits, const QuantSpec& s, int32_t* emax_dev,
          float* stats_out, void* workspace, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    QuantPartial* part = static_cast<QuantPartial*>(workspace);
    const unsigned grid = grid_of(n);
    const int rc = with_dtype(dtype, aligned16(x), [&](auto dt, auto wide) {
        typedef decltype(dt) DT;
        BSMM_LAUNCH((quant_stats_kernel<DT, wide>), grid, 256, st, static_cast<const typename DT::T*>(x), (uint32_t)n, groups_of(n), from_spec, sat_bits,
                    ftz_bits, s, emax_dev, part);
        return (int)BSMM_OK;
    });
    if (rc != BSMM_OK) return rc;
    BSMM_LAUNCH(quant_finalize_kernel, 1, 256, st, part, (int)grid, (uint32_t)n, stats_out, from_spec ? emax_dev : nullptr, s);
    return BSMM_OK;
}

inline uint32_t float_bits(float v) {
    uint32_t b;
    __builtin_memcpy(&b, &v, sizeof(b));
    return b;
}

}  // namespace

extern "C" {

size_t bsmm_quant_workspace_bytes(int64_t n) { return n_ok(n) ? (size_t)grid_of(n) * sizeof(QuantPartial) : 0; }

int bsmm_quantize(const void* x, void* y, const uint64_t* state, const int32_t* emax_dev, int64_t n, const bsmm_quant_args* args) {
    if (int rc = check_spec(args)) return rc;
    if (x == nullptr || y == nullptr || !n_ok(n)) return BSMM_ERR_ARG;
    if (args->round_mode < 0 || args->round_mode > 2 || (args->group != 0 && args->group != BSMM_QUANT_GROUP)) return BSMM_ERR_ARG;
    if (args->group != 0 && n % BSMM_QUANT_GROUP != 0) return BSMM_ERR_ARG;
    if (args->round_mode == BSMM_QUANT_STOCHASTIC && (state == nullptr || !aligned_to(state, 8))) return BSMM_ERR_ARG;
    if (emax_dev != nullptr && !aligned_to(emax_dev, 4)) return BSMM_ERR_ARG;
    if (args->dtype == BSMM_BF16 && args->fbits > 7) return BSMM_ERR_ARG;
    if (args->dtype == BSMM_F16) return BSMM_ERR_UNSUPPORTED;
    if (!aligned_to(x, args->dtype == BSMM_F32 ? 4 : 2) || !aligned_to(y, args->dtype == BSMM_F32 ? 4 : 2)) return BSMM_ERR_ARG;
    hipStream_t st = static_cast<hipStream_t>(args->stream);
    const QuantSpec s = spec_of(args);
    return with_dtype(args->dtype, aligned16(x) && aligned16(y), [&](auto dt, auto wide) {
        typedef decltype(dt) DT;
        const typename DT::T* xp = static_cast<const typename DT::T*>(x);
        typename DT::T* yp = static_cast<typename DT::T*>(y);
        const uint32_t total = (uint32_t)n, groups = groups_of(n);
        if (s.round_mode == BSMM_QUANT_NEAREST_AWAY) BSMM_LAUNCH((quant_kernel<DT, wide, BSMM_QUANT_NEAREST_AWAY>), grid_of(n), 256, st, xp, yp, state, emax_dev, s, total, groups);
        else if (s.round_mode == BSMM_QUANT_NEAREST_EVEN) BSMM_LAUNCH((quant_kernel<DT, wide, BSMM_QUANT_NEAREST_EVEN>), grid_of(n), 256, st, xp, yp, state, emax_dev, s, total, groups);
        else BSMM_LAUNCH((quant_kernel<DT, wide, BSMM_QUANT_STOCHASTIC>), grid_of(n), 256, st, xp, yp, state, emax_dev, s, total, groups);
        return (int)BSMM_OK;
    });
}

int bsmm_tensor_stats(const void* x, int64_t n, int32_t dtype, float sat_val, float ftz_val, float* stats_out, void* workspace, size_t workspace_bytes,
                      void* stream) {
    if (x == nullptr || stats_out == nullptr || !n_ok(n) || !dtype_ok(dtype) || !aligned_to(stats_out, 4)) return BSMM_ERR_ARG;
    if (!(sat_val >= 0.f) || !(ftz_val >= 0.f)) return BSMM_ERR_ARG;
    if (int rc = check_workspace(workspace, workspace_bytes, n)) return rc;
    return stats(x, n, dtype, 0, float_bits(sat_val) & 0x7fffffffu, float_bits(ftz_val) & 0x7fffffffu, QuantSpec{}, nullptr, stats_out, workspace, stream);
}

int bsmm_quant_update_emax(const void* x, int64_t n, const bsmm_quant_args* args, int32_t* emax_dev, float* stats_out) {
    if (int rc = check_spec(args)) return rc;
    if (x == nullptr || emax_dev == nullptr || !n_ok(n) || !aligned_to(emax_dev, 4)) return BSMM_ERR_ARG;
    if ((args->stat_mode != 0 && args->stat_mode != 1) || !(args->stdv_mul == args->stdv_mul)) return BSMM_ERR_ARG;
    if (stats_out != nullptr && !aligned_to(stats_out, 4)) return BSMM_ERR_ARG;
    if (args->dtype == BSMM_BF16 && args->fbits > 7) return BSMM_ERR_ARG;
    if (int rc = check_workspace(args->workspace, args->workspace_bytes, n)) return rc;
    return stats(x, n, args->dtype, 1, 0u, 0u, spec_of(args), emax_dev, stats_out, args->workspace, args->stream);
}

}  // extern "C"
