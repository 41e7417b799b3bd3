// qe_common.h -- shared host/device helpers of the gfx950 quant engine.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "qe_request.hpp"          // quant_engine.h and the host-only request checks

namespace qe {

// last failing hipError_t on this thread (qe_last_hip_error()).
extern thread_local int g_last_hip_error;

inline int hip_fail(hipError_t e) {
    g_last_hip_error = (int)e;
    return QE_ERR_HIP;
}

#define QE_HIP_TRY(expr)                                  \
    do {                                                  \
        hipError_t _e = (expr);                           \
        if (_e != hipSuccess) return ::qe::hip_fail(_e);  \
    } while (0)

// Kernel launches are followed by hipGetLastError() (the reference never checks).
#define QE_LAUNCH_CHECK() QE_HIP_TRY(hipGetLastError())

// Tuning knobs (QE_* environment variables) are read ONCE per process into a snapshot (a conv call used to make 18 getenv
// calls); env_get() answers from it.  qe_debug_reload_env() (not part of the public ABI) re-reads the environment: a test
// or an A/B tool that flips a knob inside a live process does it with quantize_amd.capi.knobs, which re-reads after setting
// the knob and again after putting the environment back.
const char *env_get(const char *name);

constexpr int kWave = 64;          // CDNA wavefront
constexpr int kNumCU = 256;        // MI355X
constexpr int kNumXCD = 8;

// One kernel instance: more than 64 KB of dynamic LDS needs the attribute, raised once per instance (to `lds_attr`; 0: the
// instance stays inside the default limit), then the launch
template <auto KERNEL, class Args>
inline void launch_instance(unsigned blocks, unsigned threads, size_t lds, size_t lds_attr, hipStream_t s, const Args &a)
{
    if (lds_attr > 0) {
        static const bool raised = hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       (int)lds_attr) == hipSuccess;
        (void)raised;
    }
    hipLaunchKernelGGL(KERNEL, dim3(blocks), dim3(threads), lds, s, a);
}

// Element `ele_idx` of a packed n_bits stream as the integer it denotes (quantconv2d.cu:103-112 / :118-127 with 64-bit
// indices): what the order-preserving kernels (qe_conv_generic.hip, the plain depthwise kernel of qe_conv_dw.hip) read with.
__device__ __forceinline__ int unpack_elem(const uint8_t *__restrict__ p, int64_t ele_idx, int n_bits, int sign)
{
    const int64_t bit = ele_idx * n_bits;
    const int64_t byte_idx = bit >> 3;
    const int bit_idx = (int)(bit & 7);
    unsigned v = ((unsigned)p[byte_idx] >> bit_idx) & ((1u << n_bits) - 1u);
    if (bit_idx + n_bits > 8) v |= ((unsigned)p[byte_idx + 1] << (8 - bit_idx)) & ((1u << n_bits) - 1u);
    const unsigned offset = sign ? (1u << (n_bits - 1)) : 0u;
    v = (v - offset) & 0xffu;
    return sign ? (int)(int8_t)v : (int)v;
}

__host__ __device__ inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

}  // namespace qe
