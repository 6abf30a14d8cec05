// pt_variance.hpp — the per-pixel variance of a frame's mean, from the frame's own sample windows.
// pt_render_device_samples renders a frame of N samples in K windows and leaves per-element running sums in d_out
// between them; differencing those sums window by window gives K batch sums, and from them the variance of each
// element's mean (the method of batch means).  No render kernel changes: this is a pass of its own, run on d_out
// right after each window, in f64 with one fixed order of operations, so the GPU, the host build
// (tests/native/Makefile) and the numpy restatement (tests/varianceref.py) give the same bits.
//
// An element is one double of d_out (a channel of a pixel; d_out's layout, the shard layout included).  Window k of
// K covers samples [e_{k-1}, e_k), e_k = (uint64)k * N / K, n_k = e_k - e_{k-1}.  Per element, with the two doubles
// of workspace prev and q, after window k's render (first: k == 1, last: k == K):
//   S    = last ? out * (double)N : out      the last window wrote the mean, so S is then the mean times N: the
//                                            rounded quotient multiplied back, not the exact sum of the samples
//   b    = first ? S : S - prev              the window's batch sum
//   t    = (b * b) / (double)n_k
//   q    = first ? t : q + t
//   prev = S
//   last: m2 = q - (S * S) / (double)N       sum over k of n_k * (mean_k - mean)^2
//         variance = (m2 > 0 ? m2 : 0) / D   D = (double)(K - 1) * (double)N, computed by the host
// The plane is the variance of the element's mean; its square root is the standard error.  An element whose samples
// are all equal can round m2 below 0: it is clamped.  A padding element of a shard has zero sums and variance 0.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pt_dims.hpp"

namespace pt {

constexpr size_t VARIANCE_WORK_PLANES = 2;  // prev, then q: `count` doubles each

namespace dev {

// One window's constants, in double, from the host (variance_consts).
struct VarConsts {
    double nk;  // (double)n_k
    double n;   // (double)N
    double d;   // (double)(K - 1) * (double)N
};

// One element after one window: reads out, updates prev and q (not read when FIRST), and with LAST returns the
// variance through *var.
template <bool FIRST, bool LAST>
PT_HD void variance_element(double out, const VarConsts &k, double *prev, double *q, double *var) {
    const double S = LAST ? out * k.n : out;
    const double b = FIRST ? S : S - *prev;
    const double t = (b * b) / k.nk;
    const double qn = FIRST ? t : *q + t;
    *q = qn;
    *prev = S;
    if (LAST) {
        const double m2 = qn - (S * S) / k.n;
        *var = (m2 > 0.0 ? m2 : 0.0) / k.d;
    }
}

}  // namespace dev

inline dev::VarConsts variance_consts(uint32_t n_k, uint32_t samples, uint32_t windows) {
    return dev::VarConsts{(double)n_k, (double)samples, (double)(windows - 1) * (double)samples};
}

// The end of window k of K over N samples (k = 0: 0; k = K: N).
inline uint32_t variance_edge(uint32_t k, uint32_t samples, uint32_t windows) {
    return (uint32_t)((uint64_t)k * samples / windows);
}

// Doubles of workspace for `count` elements; 0 when the size does not fit.
inline size_t variance_workspace_doubles(uint64_t count) {
    if (count > (uint64_t)SIZE_MAX / (VARIANCE_WORK_PLANES * sizeof(double))) return 0;
    return (size_t)count * VARIANCE_WORK_PLANES;
}

// One window's accumulation over `count` elements of out, queued on st: one launch, no host sync, no allocation, no
// atomics, no LDS.  work holds 2 * count doubles; variance (count doubles) is written only with last.  The arguments
// are checked by the caller (pt_api.cpp).
hipError_t launch_variance_window(const double *out, size_t count, const dev::VarConsts &k, bool first, bool last,
                                  double *work, double *variance, hipStream_t st);

}  // namespace pt
