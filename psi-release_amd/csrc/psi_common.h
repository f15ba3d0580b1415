// Shared host-side helpers for libpsi_hip.so (gfx950 only; no other backend exists in this build).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/psi_hip.h"

#define PSI_WAVE 64

// The Chamfer squared distance d = x2*x2 + y2*y2 + z2*z2 (chamfer.cu:32-35) in the library's two arithmetic modes:
//   default            ((x2*x2 + y2*y2) + z2*z2), three products and two sums, each rounded (the sources that use this macro
//                      are compiled with contraction off) — what the CUDA source says, i.e. nvcc --fmad=false;
//   -DPSI_CHAMFER_FMA  fma(z2, z2, fma(y2, y2, x2*x2)) — what nvcc's DEFAULT --fmad=true makes of the same expression (it
//                      contracts each `product + sum` pair left to right: mul, fma, fma).  Built as libpsi_hip_fma.so and selected
//                      with PSI_CHAMFER_FMA=1; the oracle has the matching mode (oracle/chamfer_oracle.c, same macro).
#ifdef PSI_CHAMFER_FMA
#define PSI_SQ3(x, y, z) __builtin_fmaf((z), (z), __builtin_fmaf((y), (y), (x) * (x)))
#else
#define PSI_SQ3(x, y, z) ((x) * (x) + (y) * (y) + (z) * (z))
#endif

void psi_set_error(const char *fmt, ...);

#define PSI_CHECK_HIP(expr)                                                              \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            psi_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return (int)_e;                                                              \
        }                                                                                \
    } while (0)

#define PSI_CHECK_LAUNCH(name)                                                           \
    do {                                                                                 \
        hipError_t _e = hipGetLastError();                                               \
        if (_e != hipSuccess) {                                                          \
            psi_set_error("launch of %s failed: %s", name, hipGetErrorString(_e));       \
            return (int)_e;                                                              \
        }                                                                                \
    } while (0)

#define PSI_REQUIRE(cond, msg)                                                           \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            psi_set_error("invalid argument: %s (%s)", msg, #cond);                      \
            return PSI_EINVAL;                                                           \
        }                                                                                \
    } while (0)

static inline int psi_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// n values of src in fresh device memory at *out (synchronous).  When the copy fails nothing stays allocated, *out is null and the message
// names `who`, the caller's entry point.
template <typename T>
static inline int psi_upload(T **out, const T *src, size_t n, const char *who)
{
    T *d = nullptr;
    *out = nullptr;
    PSI_CHECK_HIP(hipMalloc((void **)&d, n * sizeof(T)));
    hipError_t e = hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        psi_set_error("%s: upload failed: %s", who, hipGetErrorString(e));
        (void)hipFree(d);
        return (int)e;
    }
    *out = d;
    return 0;
}

// PSI_EINVAL unless every index of h_faces [F,3] lies in [0, V)
static inline int psi_check_faces(const int32_t *h_faces, int V, int F)
{
    for (long long k = 0; k < (long long)F * 3; k++)
        if (h_faces[k] < 0 || h_faces[k] >= V) {
            psi_set_error("invalid argument: face %lld refers to vertex %d outside [0, %d)", k / 3, (int)h_faces[k], V);
            return PSI_EINVAL;
        }
    return 0;
}

// The non-finite flag of a body-box kernel (wg_body_box in wg_device.h) before its launch: 0x7f7f7f7f, above every body index
static inline hipError_t psi_reset_bad_flag(int32_t *d_bad, hipStream_t st) { return hipMemsetAsync(d_bad, 0x7f, sizeof(int32_t), st); }

// Per-device scratch that grows on demand (used when the caller passes workspace == NULL).
void *psi_scratch(size_t bytes, hipStream_t stream);
