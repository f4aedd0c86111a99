// The plant-program interpreter (lmpc_plant_program of include/lmpc_hip.h): ONE function for both sides, like
// philox4x32_10 -- the device kernels and lmpc_plant_program_eval_host execute this source under -ffp-contract=off.
// Every operation is one IEEE binary64 operation; sine and cosine are the sequence the public header states, not the
// device library's.
//
// The interpreter knows nothing of where its operands live: an `Env` supplies
//     double slot(int s) / void set(int s, double v)      the slot file (device: LDS, [slot][lane]; host: an array)
//     double x(int a), u(int a), d(int a), q(int a)       the inputs
// The instruction stream and the constants are read at addresses that do not depend on the lane: on the device every
// lane of a wavefront executes the same instruction (no divergence), and there is no runtime-indexed private array.
// lmpc_plant_program_check (lmpc_nonlinear.hip) is what makes every index here in range; nothing is checked again.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmpc_hip.h"

namespace lmpc {

// the program as the interpreter takes it (device: ins and consts in device memory)
struct PlantProg {
    const int32_t *ins;               // n_ins x 5: op, dst, a, b, c
    const double *consts;
    int n_ins, n_slots, nx, nu, nd, nq;
};

#if defined(__HIP_DEVICE_COMPILE__)
#define LMPC_PP_ADD(a, b) __dadd_rn((a), (b))
#define LMPC_PP_SUB(a, b) __dsub_rn((a), (b))
#define LMPC_PP_MUL(a, b) __dmul_rn((a), (b))
#define LMPC_PP_DIV(a, b) __ddiv_rn((a), (b))
#define LMPC_PP_FMA(a, b, c) __fma_rn((a), (b), (c))
#else
#define LMPC_PP_ADD(a, b) ((a) + (b))
#define LMPC_PP_SUB(a, b) ((a) - (b))
#define LMPC_PP_MUL(a, b) ((a) * (b))
#define LMPC_PP_DIV(a, b) ((a) / (b))
#define LMPC_PP_FMA(a, b, c) __builtin_fma((a), (b), (c))
#endif

__host__ __device__ __forceinline__ double pp_bits(uint64_t b) { return __builtin_bit_cast(double, b); }
__host__ __device__ __forceinline__ double pp_neg(double a) { return pp_bits(__builtin_bit_cast(uint64_t, a) ^ 0x8000000000000000ull); }
__host__ __device__ __forceinline__ double pp_abs(double a) { return pp_bits(__builtin_bit_cast(uint64_t, a) & 0x7fffffffffffffffull); }

// sn and cs of the reduced argument and the quadrant m in {-2, -1, 0, 1, 2}: the header's sequence, line for line
__host__ __device__ __forceinline__ void pp_sincos(double t, double &sn, double &cs, double &m) {
    const double kd = __builtin_rint(LMPC_PP_MUL(t, pp_bits(0x3FE45F306DC9C883ull)));
    const double nk = pp_neg(kd);
    double r = LMPC_PP_FMA(nk, pp_bits(0x3FF921FB54400000ull), t);
    r = LMPC_PP_FMA(nk, pp_bits(0x3DD0B4611A600000ull), r);
    r = LMPC_PP_FMA(nk, pp_bits(0x3BA3198A2E037073ull), r);
    const double z = LMPC_PP_MUL(r, r);
    double ps = pp_bits(0x3DE5D93A5ACFD57Cull);
    ps = LMPC_PP_FMA(ps, z, pp_bits(0xBE5AE5E68A2B9CEBull));
    ps = LMPC_PP_FMA(ps, z, pp_bits(0x3EC71DE357B1FE7Dull));
    ps = LMPC_PP_FMA(ps, z, pp_bits(0xBF2A01A019C161D5ull));
    ps = LMPC_PP_FMA(ps, z, pp_bits(0x3F8111111110F8A6ull));
    ps = LMPC_PP_FMA(ps, z, pp_bits(0xBFC5555555555549ull));
    sn = LMPC_PP_FMA(LMPC_PP_MUL(r, z), ps, r);
    double pc = pp_bits(0xBDA8FAE9BE8838D4ull);
    pc = LMPC_PP_FMA(pc, z, pp_bits(0x3E21EE9EBDB4B1C4ull));
    pc = LMPC_PP_FMA(pc, z, pp_bits(0xBE927E4F809C52ADull));
    pc = LMPC_PP_FMA(pc, z, pp_bits(0x3EFA01A019CB1590ull));
    pc = LMPC_PP_FMA(pc, z, pp_bits(0xBF56C16C16C15177ull));
    pc = LMPC_PP_FMA(pc, z, pp_bits(0x3FA555555555554Cull));
    const double hz = LMPC_PP_MUL(0.5, z);
    const double w = LMPC_PP_SUB(1.0, hz);
    cs = LMPC_PP_ADD(w, LMPC_PP_FMA(LMPC_PP_MUL(z, z), pc, LMPC_PP_SUB(LMPC_PP_SUB(1.0, w), hz)));
    m = LMPC_PP_SUB(kd, LMPC_PP_MUL(4.0, __builtin_rint(LMPC_PP_MUL(0.25, kd))));
}

__host__ __device__ __forceinline__ double pp_sin(double t) {
    double sn, cs, m;
    pp_sincos(t, sn, cs, m);
    return m == 0.0 ? sn : m == 1.0 ? cs : m == -1.0 ? pp_neg(cs) : pp_neg(sn);
}

__host__ __device__ __forceinline__ double pp_cos(double t) {
    double sn, cs, m;
    pp_sincos(t, sn, cs, m);
    return m == 0.0 ? cs : m == 1.0 ? pp_neg(sn) : m == -1.0 ? sn : pp_neg(cs);
}

// run the program once on the environment's inputs; afterwards slot out_slot[a] holds x+_a
template <class Env>
__host__ __device__ __forceinline__ void plant_program_run(const PlantProg &P, Env &E) {
    for (int pc = 0; pc < P.n_ins; pc++) {
        const int32_t *I = P.ins + 5 * pc;
        const int op = I[0], dst = I[1], a = I[2], b = I[3], c = I[4];
        double v;
        switch (op) {
            case LMPC_PLANT_LOADX: v = E.x(a); break;
            case LMPC_PLANT_LOADU: v = E.u(a); break;
            case LMPC_PLANT_LOADD: v = E.d(a); break;
            case LMPC_PLANT_LOADQ: v = E.q(a); break;
            case LMPC_PLANT_CONST: v = P.consts[a]; break;
            case LMPC_PLANT_ADD: v = LMPC_PP_ADD(E.slot(a), E.slot(b)); break;
            case LMPC_PLANT_SUB: v = LMPC_PP_SUB(E.slot(a), E.slot(b)); break;
            case LMPC_PLANT_MUL: v = LMPC_PP_MUL(E.slot(a), E.slot(b)); break;
            case LMPC_PLANT_DIV: v = LMPC_PP_DIV(E.slot(a), E.slot(b)); break;
            case LMPC_PLANT_NEG: v = pp_neg(E.slot(a)); break;
            case LMPC_PLANT_ABS: v = pp_abs(E.slot(a)); break;
            case LMPC_PLANT_FMA: v = LMPC_PP_FMA(E.slot(a), E.slot(b), E.slot(c)); break;
            case LMPC_PLANT_MIN: { const double p = E.slot(a), r = E.slot(b); v = p < r ? p : r; break; }
            case LMPC_PLANT_MAX: { const double p = E.slot(a), r = E.slot(b); v = p > r ? p : r; break; }
            case LMPC_PLANT_SIN: v = pp_sin(E.slot(a)); break;
            default: v = pp_cos(E.slot(a)); break;     // LMPC_PLANT_COS: the check admits no other opcode
        }
        E.set(dst, v);
    }
}

// the host environment: one scenario's records and a slot array
struct PlantHostEnv {
    const double *xr, *ur, *dr, *qr;
    double *s;
    double slot(int i) const { return s[i]; }
    void set(int i, double v) { s[i] = v; }
    double x(int a) const { return xr[a]; }
    double u(int a) const { return ur[a]; }
    double d(int a) const { return dr[a]; }
    double q(int a) const { return qr[a]; }
};

}  // namespace lmpc
