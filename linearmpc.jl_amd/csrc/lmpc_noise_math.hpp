// The stated functions of the Gaussian draw (include/lmpc_hip.h, "GAUSSIAN draws"): ONE source for both sides, like
// philox4x32_10 and pp_sincos -- the device kernels and lmpc_noise_draw_host execute these lines under
// -ffp-contract=off.  Every operation is one IEEE binary64 operation (the LMPC_PP_* macros of lmpc_plant_program.hpp);
// the logarithm is the sequence the public header states, not the device library's, and the square root is the one
// correctly rounded binary64 square root of either side.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmpc_plant_program.hpp"

namespace lmpc {

#if defined(__HIP_DEVICE_COMPILE__)
#define LMPC_NM_SQRT(a) __dsqrt_rn((a))
#else
#define LMPC_NM_SQRT(a) __builtin_sqrt((a))
#endif

// log_(t) for t in [2^-53, 1] (normal numbers: no subnormal, zero, inf or NaN handling): the header's sequence, line
// for line.  The split is exact integer work on the bits: t = 2^k * m with m in [sqrt(2)/2, sqrt(2)).
__host__ __device__ __forceinline__ double nm_log(double t) {
    const uint64_t b = __builtin_bit_cast(uint64_t, t);
    uint32_t hx = (uint32_t)(b >> 32) + 0x00095F62u;               // + (0x3FF00000 - 0x3FE6A09E)
    const int k = (int)(hx >> 20) - 0x3FF;
    hx = (hx & 0x000FFFFFu) + 0x3FE6A09Eu;
    const double m = pp_bits(((uint64_t)hx << 32) | (b & 0xFFFFFFFFull));
    const double f = LMPC_PP_SUB(m, 1.0);                          // exact
    const double s = LMPC_PP_DIV(f, LMPC_PP_ADD(2.0, f));
    const double z = LMPC_PP_MUL(s, s);
    double p = pp_bits(0x3FC2F112DF3E5244ull);
    p = LMPC_PP_FMA(p, z, pp_bits(0x3FC39A09D078C69Full));
    p = LMPC_PP_FMA(p, z, pp_bits(0x3FC7466496CB03DEull));
    p = LMPC_PP_FMA(p, z, pp_bits(0x3FCC71C51D8E78AFull));
    p = LMPC_PP_FMA(p, z, pp_bits(0x3FD2492494229359ull));
    p = LMPC_PP_FMA(p, z, pp_bits(0x3FD999999997FA04ull));
    p = LMPC_PP_FMA(p, z, pp_bits(0x3FE5555555555593ull));
    const double R = LMPC_PP_MUL(p, z);
    const double hf = LMPC_PP_MUL(LMPC_PP_MUL(0.5, f), f);
    const double dk = (double)k;
    const double lo = LMPC_PP_ADD(LMPC_PP_MUL(s, LMPC_PP_ADD(hf, R)), LMPC_PP_MUL(dk, pp_bits(0x3DEA39EF35793C76ull)));
    return LMPC_PP_SUB(LMPC_PP_MUL(dk, pp_bits(0x3FE62E42FEE00000ull)), LMPC_PP_SUB(LMPC_PP_SUB(hf, lo), f));
}

// the standard normal pair of one Philox block (Box-Muller) from ua = philox_unit(r0, r1), ub = philox_unit(r2, r3), both
// multiples of 2^-53 in [0, 1): z0 = rho * cos_(t), z1 = rho * sin_(t).  u1 is a multiple of 2^-53 in (0, 1], so
// -2 log(u1) <= 106 ln 2 and |z| <= sqrt(106 ln 2) = 8.5717...
__host__ __device__ __forceinline__ void nm_gauss_pair(double ua, double ub, double &z0, double &z1) {
    const double u1 = LMPC_PP_SUB(1.0, ua);                        // exact, (0, 1]
    const double t = LMPC_PP_MUL(pp_bits(0x401921FB54442D18ull), ub);
    const double rho = LMPC_NM_SQRT(LMPC_PP_MUL(-2.0, nm_log(u1)));
    double sn, cs, m;
    pp_sincos(t, sn, cs, m);
    const double c = m == 0.0 ? cs : m == 1.0 ? pp_neg(sn) : m == -1.0 ? sn : pp_neg(cs);
    const double s = m == 0.0 ? sn : m == 1.0 ? cs : m == -1.0 ? pp_neg(cs) : pp_neg(sn);
    z0 = LMPC_PP_MUL(rho, c);
    z1 = LMPC_PP_MUL(rho, s);
}

// e = mean + std * z, a separate multiply and add, no clamp
__host__ __device__ __forceinline__ double nm_gauss_value(double mean, double std, double z) {
    return LMPC_PP_ADD(mean, LMPC_PP_MUL(std, z));
}

}  // namespace lmpc
