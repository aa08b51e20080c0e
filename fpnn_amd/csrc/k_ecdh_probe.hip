// k_ecdh_probe.hip -- TEST INFRASTRUCTURE ONLY (like the audit library): runs the device
// field and point functions of ecc_field.hpp one at a time, so that tests/test_gpu_ecc_field.py
// can compare the compiled device code -- folds, carry chains, product scans, inversion
// chains, the co-Z formulas -- with big-integer arithmetic on chosen operands.  Built into
// its own library (../libfpnn_ecc_probe.so = this file + k_ecdh.hip's host side for
// ecc_fill_const); the product libraries neither contain nor load it.
//
// One lane handles one operand tuple ("row").  Every field element is NW little-endian
// 32-bit limbs (NW = 8, 8, 7, 6 for ECC_SECP256K1, _SECP256R1, _SECP224R1, _SECP192R1);
// rows are packed without padding.  Limbs per row of a / b / out, in units of NW unless
// stated (b may be NULL where its row is 0):
//
//   op                      a row            b row        out row
//   ECCP_MUL                a                b            a * b
//   ECCP_SQR                a                -            a^2
//   ECCP_DUAL_MM            a1, a2           b1, b2       a1 * b1, a2 * b2     fdual<false, false>
//   ECCP_DUAL_MS            a1, a2           b1, (any)    a1 * b1, a2^2        fdual<false, true>
//   ECCP_DUAL_SM            a1, a2           (any), b2    a1^2,    a2 * b2     fdual<true, false>
//   ECCP_DUAL_SS            a1, a2           (any, any)   a1^2,    a2^2        fdual<true, true>
//   ECCP_DUAL_SS_ALIAS      a1, a2           -            a1^2,    a2^2        fdual(t5, t5, t5, s2, Y2, Y2)
//   ECCP_DUAL_MM_ALIAS      a1, a2           b1           a1 * b1, a2 * b1     fdual(X1, X1, t5, X2, X2, t5)
//   ECCP_ADD / ECCP_SUB     a                b            a + b / a - b  (a, b < p)
//   ECCP_HALF               a                -            a / 2          (a < p)
//   ECCP_REDUCE             t (NW), top (1 limb: 0 or 1)  -   reduce_once: t + top 2^(32 NW) < 2p -> mod p
//   ECCP_INV                a                -            a^(p - 2)
//   ECCP_FOLD               t (2 NW limbs)   -            fold_nf: t mod p  (t < p^2)
//   ECCP_DBL                X, Y, Z          -            X, Y, Z of dbl_jacobian (Z != 0 not checked)
//   ECCP_APPLYZ             X, Y             Z            X Z^2, Y Z^3
//   ECCP_XYCZ_ADD           X1, Y1, X2, Y2   -            X1, Y1, X2, Y2 after xycz_add
//   ECCP_XYCZ_ADDC          X1, Y1, X2, Y2   -            X1, Y1, X2, Y2 after xycz_addc
//
// The alias rows call fdual with the argument aliasing that xycz_add / xycz_addc use (a result
// object that is also an operand).  The curve constants reach the kernel as k_ecdh's do: one
// EccConst kernel argument from ecc_fill_const.
#include "ecc.hpp"

namespace fpnn_aes {

namespace {

#include "ecc_field.hpp"

enum : int {
    ECCP_MUL = 0,
    ECCP_SQR = 1,
    ECCP_DUAL_MM = 2,
    ECCP_DUAL_MS = 3,
    ECCP_DUAL_SM = 4,
    ECCP_DUAL_SS = 5,
    ECCP_DUAL_SS_ALIAS = 6,
    ECCP_DUAL_MM_ALIAS = 7,
    ECCP_ADD = 8,
    ECCP_SUB = 9,
    ECCP_HALF = 10,
    ECCP_REDUCE = 11,
    ECCP_INV = 12,
    ECCP_FOLD = 13,
    ECCP_DBL = 14,
    ECCP_APPLYZ = 15,
    ECCP_XYCZ_ADD = 16,
    ECCP_XYCZ_ADDC = 17,
    ECCP_NOPS = 18
};

// limbs per row of a / b / out: {NW multiples, extra limbs}
struct ProbeRows {
    int a_nw, a_extra, b_nw, out_nw;
};
__host__ __device__ constexpr ProbeRows probe_rows(int op) {
    switch (op) {
        case ECCP_MUL: case ECCP_ADD: case ECCP_SUB: return {1, 0, 1, 1};
        case ECCP_SQR: case ECCP_HALF: case ECCP_INV: return {1, 0, 0, 1};
        case ECCP_DUAL_MM: case ECCP_DUAL_MS: case ECCP_DUAL_SM: case ECCP_DUAL_SS: return {2, 0, 2, 2};
        case ECCP_DUAL_SS_ALIAS: return {2, 0, 0, 2};
        case ECCP_DUAL_MM_ALIAS: return {2, 0, 1, 2};
        case ECCP_REDUCE: return {1, 1, 0, 1};
        case ECCP_FOLD: return {2, 0, 0, 1};
        case ECCP_DBL: return {3, 0, 0, 3};
        case ECCP_APPLYZ: return {2, 0, 1, 2};
        default: return {4, 0, 0, 4};  // ECCP_XYCZ_ADD, ECCP_XYCZ_ADDC
    }
}

template <int NW>
__device__ __forceinline__ Fe<NW> load_le(const uint32_t *p) {
    Fe<NW> r;
#pragma unroll
    for (int j = 0; j < NW; j++) r.v[j] = p[j];
    return r;
}

template <int NW>
__device__ __forceinline__ void store_le(uint32_t *p, const Fe<NW> &a) {
#pragma unroll
    for (int j = 0; j < NW; j++) p[j] = a.v[j];
}

template <int NW, bool AM3, int FK>
__global__ __launch_bounds__(256) void k_ecc_probe(EccConst c, int op, uint32_t n, const uint32_t *a, const uint32_t *b,
                                                   uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;  // lanes never exchange data
    const ProbeRows rows = probe_rows(op);
    const uint32_t *pa = a + (size_t)i * (rows.a_nw * NW + rows.a_extra);
    const uint32_t *pb = b + (size_t)i * (rows.b_nw * NW);  // not read where b_nw == 0
    uint32_t *po = out + (size_t)i * (rows.out_nw * NW);
    switch (op) {  // wave-uniform
        case ECCP_MUL: store_le<NW>(po, fmul<NW, FK>(load_le<NW>(pa), load_le<NW>(pb), c)); break;
        case ECCP_SQR: store_le<NW>(po, fsqr<NW, FK>(load_le<NW>(pa), c)); break;
        case ECCP_DUAL_MM:
        case ECCP_DUAL_MS:
        case ECCP_DUAL_SM:
        case ECCP_DUAL_SS: {
            const Fe<NW> a1 = load_le<NW>(pa), a2 = load_le<NW>(pa + NW);
            const Fe<NW> b1 = load_le<NW>(pb), b2 = load_le<NW>(pb + NW);
            Fe<NW> r1, r2;
            if (op == ECCP_DUAL_MM) fdual<NW, FK, false, false>(r1, a1, b1, r2, a2, b2, c);
            else if (op == ECCP_DUAL_MS) fdual<NW, FK, false, true>(r1, a1, b1, r2, a2, b2, c);
            else if (op == ECCP_DUAL_SM) fdual<NW, FK, true, false>(r1, a1, b1, r2, a2, b2, c);
            else fdual<NW, FK, true, true>(r1, a1, b1, r2, a2, b2, c);
            store_le<NW>(po, r1);
            store_le<NW>(po + NW, r2);
            break;
        }
        case ECCP_DUAL_SS_ALIAS: {  // xycz_add / xycz_addc: fdual(t5, t5, t5, s2, Y2, Y2)
            Fe<NW> t5 = load_le<NW>(pa), s2;
            const Fe<NW> y2 = load_le<NW>(pa + NW);
            fdual<NW, FK, true, true>(t5, t5, t5, s2, y2, y2, c);
            store_le<NW>(po, t5);
            store_le<NW>(po + NW, s2);
            break;
        }
        case ECCP_DUAL_MM_ALIAS: {  // xycz_add / xycz_addc: fdual(X1, X1, t5, X2, X2, t5)
            Fe<NW> x1 = load_le<NW>(pa), x2 = load_le<NW>(pa + NW);
            const Fe<NW> t5 = load_le<NW>(pb);
            fdual<NW, FK, false, false>(x1, x1, t5, x2, x2, t5, c);
            store_le<NW>(po, x1);
            store_le<NW>(po + NW, x2);
            break;
        }
        case ECCP_ADD: store_le<NW>(po, fadd<NW>(load_le<NW>(pa), load_le<NW>(pb), c)); break;
        case ECCP_SUB: store_le<NW>(po, fsub<NW>(load_le<NW>(pa), load_le<NW>(pb), c)); break;
        case ECCP_HALF: store_le<NW>(po, fhalf<NW>(load_le<NW>(pa), c)); break;
        case ECCP_REDUCE: {
            const Fe<NW> t = load_le<NW>(pa);
            store_le<NW>(po, reduce_once<NW>(t.v, pa[NW], c));
            break;
        }
        case ECCP_INV: store_le<NW>(po, finv<NW, FK>(load_le<NW>(pa), c)); break;
        case ECCP_FOLD: {
            uint32_t t[2 * NW];
#pragma unroll
            for (int j = 0; j < 2 * NW; j++) t[j] = pa[j];
            store_le<NW>(po, fold_nf<NW, FK>(t, c));
            break;
        }
        case ECCP_DBL: {
            Fe<NW> x = load_le<NW>(pa), y = load_le<NW>(pa + NW), z = load_le<NW>(pa + 2 * NW);
            dbl_jacobian<NW, AM3, FK>(x, y, z, c);
            store_le<NW>(po, x);
            store_le<NW>(po + NW, y);
            store_le<NW>(po + 2 * NW, z);
            break;
        }
        case ECCP_APPLYZ: {
            Fe<NW> x = load_le<NW>(pa), y = load_le<NW>(pa + NW);
            apply_z<NW, FK>(x, y, load_le<NW>(pb), c);
            store_le<NW>(po, x);
            store_le<NW>(po + NW, y);
            break;
        }
        case ECCP_XYCZ_ADD:
        case ECCP_XYCZ_ADDC: {
            Fe<NW> x1 = load_le<NW>(pa), y1 = load_le<NW>(pa + NW), x2 = load_le<NW>(pa + 2 * NW),
                   y2 = load_le<NW>(pa + 3 * NW);
            if (op == ECCP_XYCZ_ADD) xycz_add<NW, FK>(x1, y1, x2, y2, c);
            else xycz_addc<NW, FK>(x1, y1, x2, y2, c);
            store_le<NW>(po, x1);
            store_le<NW>(po + NW, y1);
            store_le<NW>(po + 2 * NW, x2);
            store_le<NW>(po + 3 * NW, y2);
            break;
        }
        default: break;
    }
}

template <int NW, bool AM3, int FK>
void launch_probe(const EccConst &c, int op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out,
                  hipStream_t st) {
    hipLaunchKernelGGL((k_ecc_probe<NW, AM3, FK>), dim3((n + 255) / 256), dim3(256), 0, st, c, op, n, a, b, out);
}

}  // namespace

}  // namespace fpnn_aes

// Runs `op` of `curve` (ECC_SECP256K1 .. ECC_SECP192R1) on n rows; a, b and out are device
// pointers laid out as the table above says (b may be NULL for ops without a b row).  The
// launch is asynchronous on `st`.  Returns 0, or a hipError_t (hipErrorInvalidValue for an
// unknown curve or op, a missing pointer or n >= 2^24).
extern "C" int fpnn_ecc_probe(int curve, int op, uint32_t n, const uint32_t *a, const uint32_t *b, uint32_t *out,
                              hipStream_t st) {
    using namespace fpnn_aes;
    EccConst c;
    if (op < 0 || op >= ECCP_NOPS || !ecc_fill_const(curve, c)) return (int)hipErrorInvalidValue;
    if (n == 0) return 0;
    if (!a || !out || (!b && probe_rows(op).b_nw != 0) || n >= (1u << 24)) return (int)hipErrorInvalidValue;
    switch (curve) {
        case ECC_SECP256K1: launch_probe<8, false, FK_K1>(c, op, n, a, b, out, st); break;
        case ECC_SECP256R1: launch_probe<8, true, FK_P256>(c, op, n, a, b, out, st); break;
        case ECC_SECP224R1: launch_probe<7, true, FK_P224>(c, op, n, a, b, out, st); break;
        default: launch_probe<6, true, FK_P192>(c, op, n, a, b, out, st); break;
    }
    return (int)hipGetLastError();
}
