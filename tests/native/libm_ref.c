/* The host reference of the device libm sweep (tests/libmset.py, tests/test_gpu_libm_sweep.py, tests/test_libm.py), over arrays.
 * Function ids are rtx_debug_libm's (include/rtx.h): 0 acosf 1 atan2f 2 expf 3 log2f 4 atanf 5 cvtss2si 6 1 / sqrtf 7 cvttss2si 8 pow2<128>.
 *   ref_unary / ref_binary    REF: nothing of the project.  The host libm's acosf, atanf, atan2f, expf, log2f; 1.0f / sqrtf; the two SSE
 *                             conversions themselves (the instructions the reference executes: NaN and out-of-range give the integer
 *                             indefinite 0x80000000), returned as float like the hook does; seven plain float squarings.
 *   port_unary / port_binary  PORT: csrc/rtx_libm.h compiled for the host (ids 0 .. 4 only), for diagnosis: it tells a host libm that moved
 *                             from a device build that diverged.
 * Every function returns 0, or -1 for an id it does not know (nothing written).
 * Build: gcc -O2 -ffp-contract=off -shared -fPIC libm_ref.c -lm   (no fast-math: sqrtf and / are the correctly rounded instructions) */
#include <stdint.h>
#include <math.h>
#include <xmmintrin.h>
#include "../../cpu-raytracer_amd/csrc/rtx_libm.h"

static float ref_pow2_128(float v) {
    v = v * v; v = v * v; v = v * v; v = v * v; v = v * v; v = v * v; v = v * v;
    return v;
}

int ref_unary(int fn, const float * in, float * out, int64_t n) {
    switch (fn) {
        case 0: for (int64_t i = 0; i < n; i++) out[i] = acosf(in[i]); return 0;
        case 2: for (int64_t i = 0; i < n; i++) out[i] = expf(in[i]); return 0;
        case 3: for (int64_t i = 0; i < n; i++) out[i] = log2f(in[i]); return 0;
        case 4: for (int64_t i = 0; i < n; i++) out[i] = atanf(in[i]); return 0;
        case 5: for (int64_t i = 0; i < n; i++) out[i] = (float)_mm_cvtss_si32(_mm_set_ss(in[i])); return 0;
        case 6: for (int64_t i = 0; i < n; i++) out[i] = 1.0f / sqrtf(in[i]); return 0;
        case 7: for (int64_t i = 0; i < n; i++) out[i] = (float)_mm_cvttss_si32(_mm_set_ss(in[i])); return 0;
        case 8: for (int64_t i = 0; i < n; i++) out[i] = ref_pow2_128(in[i]); return 0;
        default: return -1;
    }
}

int ref_binary(int fn, const float * a, const float * b, float * out, int64_t n) {
    if (fn != 1) return -1;
    for (int64_t i = 0; i < n; i++) out[i] = atan2f(a[i], b[i]);
    return 0;
}

int port_unary(int fn, const float * in, float * out, int64_t n) {
    switch (fn) {
        case 0: for (int64_t i = 0; i < n; i++) out[i] = rtx_acosf(in[i]); return 0;
        case 2: for (int64_t i = 0; i < n; i++) out[i] = rtx_expf(in[i]); return 0;
        case 3: for (int64_t i = 0; i < n; i++) out[i] = rtx_log2f(in[i]); return 0;
        case 4: for (int64_t i = 0; i < n; i++) out[i] = rtx_atanf(in[i]); return 0;
        default: return -1;
    }
}

int port_binary(int fn, const float * a, const float * b, float * out, int64_t n) {
    if (fn != 1) return -1;
    for (int64_t i = 0; i < n; i++) out[i] = rtx_atan2f(a[i], b[i]);
    return 0;
}
