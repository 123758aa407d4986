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

// ---------------------------------------------------------------------------------------------------------
// device: store policy
// ---------------------------------------------------------------------------------------------------------
// A kernel's output store with its cache policy chosen at compile time.  WT = false is the plain store.  WT = true is a
// WRITE-THROUGH store (a relaxed agent-scope atomic store: `global_store_* ... sc1`, no fence and no wait added): the bytes
// leave the XCD's L2 while the kernel still runs instead of sitting there dirty until the launch's closing release writes
// them back with every SIMD idle.  For output that the launch itself never reads again and whose volume is a sizeable part
// of L2 (the env step at one wave per SIMD: 17 MB of 32); loads are not touched.
template <bool WT, typename T>
FD_DEV void put(T* p, T v)
{
    if constexpr (WT) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
// FD_PUT(WT, lvalue, value): `lvalue = value` under the policy WT, for code that is instantiated both ways.  A macro, so that
// the WT = false branch is the assignment itself: a call evaluates the address before the value, an assignment the value
// first, and with the operands born in another order the scheduler's ties fall differently -- the plain instantiations
// would no longer compile to the instructions they had before the policy existed.
#define FD_PUT(WT, dst, val) do { if constexpr (WT) fdyn::put<true>(&(dst), (val)); else (dst) = (val); } while (0)
// The 16-byte write-through store (there is no 16-byte atomic store), for a wave that writes one contiguous range: `base` and
// `bytes` are wave-uniform, `off` is the lane's byte offset inside the range; the buffer descriptor drops a lane at or past
// `bytes`.  `buffer_store_dwordx4 ... offen sc1`.
FD_DEV void put16_through(float* base, uint32_t bytes, uint32_t off, const float4& v)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    // the descriptor lives in scalar registers: say that the base is wave-uniform where the compiler cannot see it
    // (the builtin returns a signed int: each half goes through uint32_t, or a low word with bit 31 set sign-extends into
    // the high one)
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(b))));
    const uint32_t hi = uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(b >> 32))));
    base = reinterpret_cast<float*>(uint64_t(lo) | (uint64_t(hi) << 32));
    bytes = uint32_t(__builtin_amdgcn_readfirstlane(int(bytes)));
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(base, 0, int(bytes), 0x00020000);
    const u32x4 w = { __float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w) };
    __builtin_amdgcn_raw_buffer_store_b128(w, rsrc, int(off), 0, 16 /* sc1 */);
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
