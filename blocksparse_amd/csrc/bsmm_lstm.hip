// bsmm_lstm.hip -- C-ABI entry points of include/bsmm_lstm.h: argument checks, the geometry both layouts share, the choice between the
// 16-byte path and the element path (sizes and pointer alignment only), then one launch of a kernel of bsmm_lstm_kernels.h.  No allocation,
// no host sync, no environment, no state.
#include <cstdint>

#include "bsmm_lstm.h"
#include "bsmm_host.h"
#include "bsmm_lstm_kernels.h"

using namespace bsmm;

namespace {

int check(const bsmm_lstm_args* a, bool grad) {
    if (a == nullptr || a->K < 1 || a->N < 1 || !product_ok(a->K, a->N)) return BSMM_ERR_ARG;
    if ((long long)a->K * 4 >= (1ll << 31)) return BSMM_ERR_ARG;
    if ((a->axis != 0 && a->axis != 1) || !dtype_ok(a->dtype)) return BSMM_ERR_ARG;
    if (a->axis == 1 && (a->gate_ld < a->K || (grad && a->dgate_ld < a->K))) return BSMM_ERR_ARG;
    return BSMM_OK;
}

// rows x cols with contiguous rows in c; the gates gate_ld apart
struct Geom {
    uint32_t rows, cols;
    size_t gate_ld, dgate_ld;
    int by_row;
};

inline Geom geom(const bsmm_lstm_args* a) {
    Geom g;
    if (a->axis == 0) {
        g.rows = (uint32_t)a->K; g.cols = (uint32_t)a->N; g.gate_ld = g.dgate_ld = (size_t)a->N; g.by_row = 1;
    } else {
        g.rows = (uint32_t)a->N; g.cols = (uint32_t)a->K; g.gate_ld = (size_t)a->gate_ld; g.dgate_ld = (size_t)a->dgate_ld; g.by_row = 0;
    }
    return g;
}

inline unsigned grid_of(uint32_t units) { return capped((units + 255u) / 256u, LSTM_MAX_GRID); }
inline uint32_t magic_of(uint32_t upr) { return upr == 1u ? 0xffffffffu : (uint32_t)((1ull << 32) / upr); }

// elements of a 16-byte access
template <class DT>
constexpr int WIDE = DT::is16 ? 8 : 4;

template <class DT, int V>
int forward(const void* c, const void* i, const void* u, const void* f, const void* o, const float* bias, void* cn, void* hn, const Geom& g,
            const bsmm_lstm_args* a) {
    typedef typename DT::T T;
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const uint32_t upr = g.cols / V, units = g.rows * upr;
    BSMM_LAUNCH((lstm_fwd_kernel<DT, V>), grid_of(units), 256, st, static_cast<const T*>(c), static_cast<const T*>(i), static_cast<const T*>(u),
                static_cast<const T*>(f), static_cast<const T*>(o), bias, static_cast<T*>(cn), static_cast<T*>(hn), g.cols, upr, magic_of(upr), units,
                g.gate_ld, (uint32_t)a->K, g.by_row, a->forget_bias);
    return BSMM_OK;
}

template <class DT, int V>
int backward(const void* c, const void* i, const void* u, const void* f, const void* o, const float* bias, const void* eh, const void* ec, void* dc,
             void* di, void* du, void* df, void* d_o, const Geom& g, const bsmm_lstm_args* a) {
    typedef typename DT::T T;
    hipStream_t st = static_cast<hipStream_t>(a->stream);
    const uint32_t upr = g.cols / V, units = g.rows * upr;
    BSMM_LAUNCH((lstm_bwd_kernel<DT, V>), grid_of(units), 256, st, static_cast<const T*>(c), static_cast<const T*>(i), static_cast<const T*>(u),
                static_cast<const T*>(f), static_cast<const T*>(o), bias, static_cast<const T*>(eh), static_cast<const T*>(ec), static_cast<T*>(dc),
                static_cast<T*>(di), static_cast<T*>(du), static_cast<T*>(df), static_cast<T*>(d_o), g.cols, upr, magic_of(upr), units, g.gate_ld,
                g.dgate_ld, (uint32_t)a->K, g.by_row, a->forget_bias);
    return BSMM_OK;
}

}  // namespace

extern "C" {

int bsmm_lstm_gates(const void* c, const void* i, const void* u, const void* f, const void* o, const float* bias, void* c_next, void* h_next,
                    const bsmm_lstm_args* args) {
    if (int rc = check(args, false)) return rc;
    if (c == nullptr || i == nullptr || u == nullptr || f == nullptr || o == nullptr || c_next == nullptr || h_next == nullptr) return BSMM_ERR_ARG;
    const Geom g = geom(args);
    const uint32_t V = args->dtype == BSMM_F32 ? 4u : 8u;
    const bool wide = g.cols % V == 0 && g.gate_ld % V == 0 && aligned16(c) && aligned16(i) && aligned16(u) && aligned16(f) && aligned16(o) &&
                      aligned16(c_next) && aligned16(h_next);
    return with_dtype(args->dtype, wide, [&](auto dt, auto w) {
        return forward<decltype(dt), (w ? WIDE<decltype(dt)> : 1)>(c, i, u, f, o, bias, c_next, h_next, g, args);
    });
}

int bsmm_lstm_gates_grad(const void* c, const void* i, const void* u, const void* f, const void* o, const float* bias, const void* eh, const void* ec,
                         void* dc, void* di, void* du, void* df, void* d_o, const bsmm_lstm_args* args) {
    if (int rc = check(args, true)) return rc;
    if (c == nullptr || i == nullptr || u == nullptr || f == nullptr || o == nullptr || (eh == nullptr && ec == nullptr)) return BSMM_ERR_ARG;
    if (dc == nullptr || di == nullptr || du == nullptr || df == nullptr || d_o == nullptr) return BSMM_ERR_ARG;
    const Geom g = geom(args);
    const uint32_t V = args->dtype == BSMM_F32 ? 4u : 8u;
    const bool wide = g.cols % V == 0 && g.gate_ld % V == 0 && g.dgate_ld % V == 0 && aligned16(c) && aligned16(i) && aligned16(u) && aligned16(f) &&
                      aligned16(o) && aligned16(eh) && aligned16(ec) && aligned16(dc) && aligned16(di) && aligned16(du) && aligned16(df) && aligned16(d_o);
    return with_dtype(args->dtype, wide, [&](auto dt, auto w) {
        return backward<decltype(dt), (w ? WIDE<decltype(dt)> : 1)>(c, i, u, f, o, bias, eh, ec, dc, di, du, df, d_o, g, args);
    });
}

}  // extern "C"
