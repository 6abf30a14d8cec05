// pt_variance.hip — the variance accumulation for MI355X (gfx950): the kernel of pt_variance.hpp.  Its own
// translation unit: nothing of the render path is compiled here, and this object is not part of the render path's
// identity (PT_SRC_SHA, Makefile).
#include <hip/hip_runtime.h>

#include "pt_variance.hpp"

namespace pt {

// One thread per pair of elements with WIDE (16-byte loads and stores: out, prev, q and variance are all 16-byte
// aligned and count is even; q = prev + count, so an odd count never has both aligned), else one per element.
// Plain streaming: the first window reads 8 bytes per element and writes 16, a middle one reads 24 and writes 16,
// the last one reads 24 and writes 24.  FIRST does not read the workspace, so the caller need not clear it.
// Resources (gfx950, -O3): 16 to 48 VGPRs over the six builds, 0 AGPRs, no scratch, no LDS, 8 waves per SIMD.
template <bool FIRST, bool LAST, bool WIDE>
__global__ __launch_bounds__(256) void variance_window(const double *__restrict__ out, size_t count, dev::VarConsts k,
                                                       double *__restrict__ prev, double *__restrict__ q,
                                                       double *__restrict__ variance) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (WIDE) {
        const size_t pairs = count / 2;
        if (i < pairs) {
            const double2 o = ((const double2 *)out)[i];
            double2 p = FIRST ? double2{0.0, 0.0} : ((const double2 *)prev)[i];
            double2 a = FIRST ? double2{0.0, 0.0} : ((const double2 *)q)[i];
            double2 v{0.0, 0.0};
            dev::variance_element<FIRST, LAST>(o.x, k, &p.x, &a.x, &v.x);
            dev::variance_element<FIRST, LAST>(o.y, k, &p.y, &a.y, &v.y);
            ((double2 *)prev)[i] = p;
            ((double2 *)q)[i] = a;
            if (LAST) ((double2 *)variance)[i] = v;
        }
    } else if (i < count) {
        double v = 0.0;
        dev::variance_element<FIRST, LAST>(out[i], k, &prev[i], &q[i], &v);
        if (LAST) variance[i] = v;
    }
}

template <bool FIRST, bool LAST>
static hipError_t launch_window(const double *out, size_t count, const dev::VarConsts &k, double *prev, double *q,
                                double *variance, hipStream_t st) {
    const uintptr_t bits = (uintptr_t)out | (uintptr_t)prev | (uintptr_t)q | (LAST ? (uintptr_t)variance : 0);
    const bool wide = (bits & 15u) == 0 && (count & 1u) == 0;
    const uint64_t threads = wide ? (uint64_t)count / 2 : (uint64_t)count;
    const uint64_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (wide) variance_window<FIRST, LAST, true><<<(unsigned)blocks, 256, 0, st>>>(out, count, k, prev, q, variance);
    else variance_window<FIRST, LAST, false><<<(unsigned)blocks, 256, 0, st>>>(out, count, k, prev, q, variance);
    return hipGetLastError();
}

hipError_t launch_variance_window(const double *out, size_t count, const dev::VarConsts &k, bool first, bool last,
                                  double *work, double *variance, hipStream_t st) {
    if (count == 0 || (first && last) || (last && !variance)) return hipErrorInvalidValue;
    double *prev = work, *q = work + count;
    if (first) return launch_window<true, false>(out, count, k, prev, q, variance, st);
    if (last) return launch_window<false, true>(out, count, k, prev, q, variance, st);
    return launch_window<false, false>(out, count, k, prev, q, variance, st);
}

}  // namespace pt
