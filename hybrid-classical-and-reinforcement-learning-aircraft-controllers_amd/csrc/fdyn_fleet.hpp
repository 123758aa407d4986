// fdyn_fleet.hpp -- what the fleet kernel files (fdyn_kernels.hip, lqr_kernels.hip, trim_kernels.hip) share around fdyn_core.hpp:
// the staging of the parameter blocks into LDS, the lane's aircraft type, the glue type, and on the host side the launch and
// the entry checks.  One copy, so that a change to the staged block's layout reaches every fleet at once.  Only what more than
// one of those files needs lives here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fdyn_core.hpp"
#include "../../include/fdyn.h"

namespace fdyn {

constexpr int FD_MAX_TYPES = 8;          // aircraft types per launch: the parameter blocks one workgroup stages
constexpr int FD_WAVE = 64;

// ---------------------------------------------------------------------------------------------------------
// device: LDS staging helpers
// ---------------------------------------------------------------------------------------------------------
template <typename T>
FD_DEV void stage(T* dst, const T* __restrict__ src, int n)
{
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

// Parameter blocks -> LDS: the FD_NP_USED caller words are copied; meanwhile a few threads per aircraft type fill the block's
// derived words straight from global memory, one word per lane (Params::derive_lane).  One barrier (the caller's).  Kernels
// issue their per-aircraft global loads BEFORE calling this, so the HBM round trip of the state overlaps the staging chain
// (global -> LDS -> barrier -> LDS -> registers) instead of following it.  The workgroup must have at least
// FD_MAX_TYPES * Params<double>::FD_ND_LANES threads.
template <bool FAST>
FD_DEV void stage_params(double* s_params, const double* __restrict__ params, int n_types)
{
    for (int i = threadIdx.x; i < n_types * FD_NP_USED; i += blockDim.x) {
        const int t = i / FD_NP_USED, k = i - t * FD_NP_USED;
        s_params[t * FD_NP_STAGED + k] = params[t * FD_NP + k];
    }
    constexpr int NDL = Params<double>::FD_ND_LANES;
    if (int(threadIdx.x) < n_types * NDL) {
        const int t = threadIdx.x / NDL;
        Params<double>::derive_lane<FAST>(threadIdx.x - t * NDL, params + t * FD_NP, s_params + t * FD_NP_STAGED);
    }
}

FD_DEV int lane_type(const uint8_t* __restrict__ type, int64_t i, int n_types)
{
    int t = type ? int(type[i]) : 0;
    return t < n_types ? t : n_types - 1;
}

// Glue type of the agents and control laws: the storage type for the fp64 parity variant, the COMPUTE type for the
// fp32-evaluation variants (their PIDs take fp32 inputs anyway; round 1 ran the glue in fp64 -- ocml sincos / atan2 / fmod
// several times per control step -- and the glue cost more than the physics: 7.3 us per control step of which 3.1 us were the RK4).
template <typename S, typename T> struct GlueOf { using type = S; };
template <typename S> struct GlueOf<S, float> { using type = float; };

// ---------------------------------------------------------------------------------------------------------
// host: entry checks and launch
// ---------------------------------------------------------------------------------------------------------
// simplified_6dof.py:241-245: dt <= min_timestep or > max_timestep raises ValueError (defaults)
inline bool bad_dt(double dt) { return !(dt > 1e-6) || dt > 1.0; }

// size and type count of a launch of BLOCK-lane workgroups, in the order every entry point reports them; an empty fleet is done
#define FD_CHECK_FLEET(n, n_types, BLOCK)                                           \
    if ((n) < 0 || (n) > (int64_t(1) << 31) - (BLOCK)) return FDYN_ERR_BAD_SIZE;    \
    if ((n_types) < 1 || (n_types) > FD_MAX_TYPES) return FDYN_ERR_BAD_TYPES;       \
    if ((n) == 0) return FDYN_OK;

// every fleet kernel is launched the same way: one lane per row, BLOCK lanes per workgroup, no dynamic LDS
template <int BLOCK, typename K, typename... A>
int launch(K kernel, int64_t n, void* stream, A... args)
{
    hipLaunchKernelGGL(kernel, dim3(unsigned((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, args...);
    return int(hipGetLastError());
}

}  // namespace fdyn
