// fdyn_kernels.hip -- gfx950 kernels + the C-ABI of include/fdyn.h.
//
// Mapping: one lane = one aircraft / env, 256-thread workgroups (4 wave64).  State is structure-of-arrays
// ([word][N]) so every load/store of a wave is one contiguous 256 B (fp32) / 512 B (fp64) segment.
// The aircraft "coefficient table" (one FD_NP-word block per aircraft TYPE; the reference has closed-form
// coefficients, not lookup tables) plus the PID / cascade / waypoint tables are staged in LDS once per
// workgroup; each lane then pulls its own type's block into registers, so heterogeneous fleets cost nothing
// extra in the inner loop.  All sub-steps of a launch run out of registers: HBM traffic per launch is one
// read + one write of the state.  Episode ends are compacted with a wave ballot + mbcnt prefix and ONE
// atomic per wave into a dense event list (terminal observation, return, length) -- the only inter-lane
// communication in the path; there is no inter-workgroup communication at all.
// What the other fleet files (lqr_kernels.hip, trim_kernels.hip) need as well -- parameter staging, lane type, glue type, the
// entry checks and the launch -- is in fdyn_fleet.hpp; the staging helpers that remain here are the rate env's own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <stdlib.h>
#include "fdyn_fleet.hpp"

using namespace fdyn;

#define FD_BLOCK 256

// ---------------------------------------------------------------------------------------------------------
// LDS staging helpers of the rate env (stage, stage_params: fdyn_fleet.hpp)
// ---------------------------------------------------------------------------------------------------------
// stage_params in two halves, for a kernel whose launch is one burst of per-aircraft loads (the env step at one wave per SIMD): loads
// return IN ORDER, so a parameter word requested after the state is not in LDS -- and the barrier not passed -- before the whole
// burst has landed.  `early` issues the block's loads FIRST; `finish` stores them once they are back, ahead of the state.
struct StagedParamWords { double v0, v1, d; };
__device__ __forceinline__ StagedParamWords stage_params_early(const double* __restrict__ params, int n_types)
{
    StagedParamWords w;                                           // FD_MAX_TYPES * FD_NP_USED <= 2 * FD_BLOCK: two words per thread
    const int i0 = threadIdx.x, i1 = FD_BLOCK + threadIdx.x;
    const int t0 = i0 / FD_NP_USED, t1 = i1 / FD_NP_USED;
    w.v0 = i0 < n_types * FD_NP_USED ? params[t0 * FD_NP + (i0 - t0 * FD_NP_USED)] : 0.0;
    w.v1 = i1 < n_types * FD_NP_USED ? params[t1 * FD_NP + (i1 - t1 * FD_NP_USED)] : 0.0;
    constexpr int NDL = Params<double>::FD_ND_LANES;
    const int t = threadIdx.x / NDL;
    w.d = int(threadIdx.x) < n_types * NDL ? params[t * FD_NP + Params<double>::derive_source(threadIdx.x - t * NDL)] : 1.0;
    return w;
}
template <bool FAST>
__device__ __forceinline__ void stage_params_finish(double* s_params, const StagedParamWords& w, int n_types)
{
    const int i0 = threadIdx.x, i1 = FD_BLOCK + threadIdx.x;
    const int t0 = i0 / FD_NP_USED, t1 = i1 / FD_NP_USED;
    if (i0 < n_types * FD_NP_USED) s_params[t0 * FD_NP_STAGED + (i0 - t0 * FD_NP_USED)] = w.v0;
    if (i1 < n_types * FD_NP_USED) s_params[t1 * FD_NP_STAGED + (i1 - t1 * FD_NP_USED)] = w.v1;
    constexpr int NDL = Params<double>::FD_ND_LANES;
    if (int(threadIdx.x) < n_types * NDL) {
        const int t = threadIdx.x / NDL;
        Params<double>::derive_lane_from<FAST>(threadIdx.x - t * NDL, w.d, s_params + t * FD_NP_STAGED);
    }
}

// A PREPARED parameter block (the rate env's launch image, fdyn_rate_env_image): [n_types][FD_NP_STAGED] words with the derived
// ones already in place, so staging is a plain copy -- the same two halves around the caller's per-aircraft loads.
__device__ __forceinline__ StagedParamWords stage_image_early(const double* __restrict__ staged, int n_types)
{
    StagedParamWords w;                                           // FD_MAX_TYPES * FD_NP_STAGED <= 2 * FD_BLOCK
    const int i0 = threadIdx.x, i1 = FD_BLOCK + threadIdx.x;
    w.v0 = i0 < n_types * FD_NP_STAGED ? staged[i0] : 0.0;
    w.v1 = i1 < n_types * FD_NP_STAGED ? staged[i1] : 0.0;
    w.d = 1.0;
    return w;
}
__device__ __forceinline__ void stage_image_finish(double* s_params, const StagedParamWords& w, int n_types)
{
    const int i0 = threadIdx.x, i1 = FD_BLOCK + threadIdx.x;
    if (i0 < n_types * FD_NP_STAGED) s_params[i0] = w.v0;
    if (i1 < n_types * FD_NP_STAGED) s_params[i1] = w.v1;
}

// Cascade constants -> LDS in the glue type, plus the two derived reciprocals the fp32 guidance uses
template <typename G>
__device__ __forceinline__ void stage_cascade_consts(G* s_consts, const double* __restrict__ consts)
{
    for (int k = threadIdx.x; k < FD_NC; k += blockDim.x) s_consts[k] = G(consts[k]);
    if (threadIdx.x < 2) {
        const double bank = consts[threadIdx.x == 0 ? FD_C_WP_MAX_BANK_RAD : FD_C_LOS_MAX_BANK_RAD];
        s_consts[FD_CD_WP_INV_G_TAN_BANK + threadIdx.x] = G(1.0 / (9.81 * ::tan(bank)));
    }
}

// Lane -> aircraft map: one lane = one aircraft, fully populated wave64.  (Round 1 measured half- and quarter-populated
// waves -- 32 / 16 lanes per wave to get 2 / 4 waves per SIMD at N = 65 536: 67.8 -> 99.9 / 182.7 us for the mixed env
// step.  The SIMD retires ~1 VALU per 5 cycles from one wave and ~1 per 3.4 from four, so doubling the instruction
// count to double the wave count loses; the plumbing was removed in round 2, the result stays in DESIGN.md.)
struct LaneMap { int64_t i, wave_first; int lane; bool on; };
__device__ __forceinline__ LaneMap lane_map(int64_t n)
{
    LaneMap m;
    m.lane = threadIdx.x & (FD_WAVE - 1);
    m.i = int64_t(blockIdx.x) * FD_BLOCK + threadIdx.x;
    m.wave_first = m.i - m.lane;
    m.on = m.i < n;
    return m;
}

// ---------------------------------------------------------------------------------------------------------
// K1: Simplified6DOF.step x n_sub                        (simplified_6dof.py:228-293, simulation_backend.py:95-99)
// ---------------------------------------------------------------------------------------------------------
template <typename S, typename T>
__global__ void __launch_bounds__(FD_BLOCK)
sixdof_step_kernel(S* __restrict__ xs, const S* __restrict__ us, const uint8_t* __restrict__ type,
                   const double* __restrict__ params, int n_types, int64_t n, S dt_sub, int n_sub,
                   S* __restrict__ derived_out)
{
    __shared__ double s_params[FD_MAX_TYPES * FD_NP_STAGED];
    const LaneMap lm = lane_map(n);
    const int64_t i = lm.i;
    S x[FD_NX], uc[FD_NU];
    int ty = 0;
    if (lm.on) {                                             // state / control loads in flight during the parameter staging
#pragma unroll
        for (int k = 0; k < FD_NX; ++k) x[k] = xs[k * n + i];
#pragma unroll
        for (int k = 0; k < FD_NU; ++k) uc[k] = us[k * n + i];
        ty = lane_type(type, i, n_types);
    }
    stage_params<sizeof(T) == 4>(s_params, params, n_types);
    __syncthreads();
    if (!lm.on) return;

    const double* blk = s_params + ty * FD_NP_STAGED;
    Params<T> P; P.load(blk);
    Limits<S> Lm; Lm.load(blk);
    Controls<T> C;
    C.set(P, uc[FD_U_ELEVATOR], uc[FD_U_AILERON], uc[FD_U_RUDDER], uc[FD_U_THROTTLE]);

    rk4_substeps<S, T>(P, Lm, C, x, dt_sub, n_sub);

#pragma unroll
    for (int k = 0; k < FD_NX; ++k) xs[k * n + i] = x[k];
    if (derived_out) {
        const Derived<S> d = derived<S>(x);
        derived_out[FD_D_AIRSPEED * n + i] = d.airspeed;
        derived_out[FD_D_ALTITUDE * n + i] = d.altitude;
        derived_out[FD_D_GROUND_SPEED * n + i] = d.ground_speed;
        derived_out[FD_D_HEADING * n + i] = d.heading;
    }
}

// get_state's derived scalars for a whole fleet (simplified_6dof.py:295-331)
template <typename S>
__global__ void __launch_bounds__(FD_BLOCK)
derived_kernel(const S* __restrict__ xs, int64_t n, S* __restrict__ out)
{
    const int64_t i = int64_t(blockIdx.x) * FD_BLOCK + threadIdx.x;
    if (i >= n) return;
    S x[FD_NX];
#pragma unroll
    for (int k = 0; k < FD_NX; ++k) x[k] = xs[k * n + i];
    const Derived<S> d = derived<S>(x);
    out[FD_D_AIRSPEED * n + i] = d.airspeed;
    out[FD_D_ALTITUDE * n + i] = d.altitude;
    out[FD_D_GROUND_SPEED * n + i] = d.ground_speed;
    out[FD_D_HEADING * n + i] = d.heading;
}

// ---------------------------------------------------------------------------------------------------------
// batched scalar PID (the reference's only native code, cpp/src/pid_controller.cpp:24-60), one lane per loop
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FD_BLOCK)
pid_batch_kernel(const float* __restrict__ cfg /*[8] shared or [n][8]*/, int cfg_per_lane,
                 float* __restrict__ state /*[3][n]*/, const float* __restrict__ setpoint,
                 const float* __restrict__ measurement, float dt, float* __restrict__ out, int64_t n)
{
    const int64_t i = int64_t(blockIdx.x) * FD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const PidCfg c = load_pid_cfg(cfg + (cfg_per_lane ? i * FD_NPC : 0), 0);
    PidState s{ state[FD_PS_INTEGRAL * n + i], state[FD_PS_ERR_PREV * n + i], state[FD_PS_DFILT * n + i] };
    out[i] = pid_compute(c, s, setpoint[i], measurement[i], dt);
    state[FD_PS_INTEGRAL * n + i] = s.integral;
    state[FD_PS_ERR_PREV * n + i] = s.err_prev;
    state[FD_PS_DFILT * n + i] = s.dfilt;
}

// ---------------------------------------------------------------------------------------------------------
// K1+K2: n_steps control steps of the 5-level cascade + one RK4 each
//        (examples/03_waypoint_square_demo.py:148-209 per aircraft; agents in fdyn_core.hpp)
// ---------------------------------------------------------------------------------------------------------
// Storage type of the 21 env words (`e`): the state's storage type in the f64 and f32 variants, fp32 in `mixed` -- they are
// commands, previous actions and reward-tracker state, computed in fp32 there anyway (GlueOf, fdyn_fleet.hpp); as fp64 rows they were
// 272 of the 660 bytes an env step moves.  Two words are kept exact in fp32 form: the settling timer counts STEPS (fp32
// holds small integers exactly; the threshold is the step count at which the reference's accumulated fp64 sum reaches 0.2 s)
// and the episode time is step * dt rather than an accumulated fp32 sum.
template <typename S, typename T> struct EnvOf { using type = S; };
template <> struct EnvOf<double, float> { using type = float; };

// (FD_BLOCK, 1): nine PID configurations, 27 PID states, the constants and the integrator state are ~250 live registers;
// under the default occupancy target the allocator parked part of them in AGPRs and paid ~80 v_accvgpr moves per control step
template <typename S, typename T>
__global__ void __launch_bounds__(FD_BLOCK, 1)
cascade_step_kernel(S* __restrict__ xs, float* __restrict__ pid_state /*[9*3][n]*/, int32_t* __restrict__ wp_idx,
                    const uint8_t* __restrict__ type, const double* __restrict__ params, int n_types,
                    const float* __restrict__ pid_cfg /*[9][8]*/, const double* __restrict__ consts /*[FD_NC]*/,
                    const double* __restrict__ wps /*[n_wp][4]*/, int n_wp, int64_t n, S dt, int n_steps,
                    S* __restrict__ surf_out /*[4][n] or null*/, int32_t* __restrict__ reached_total /*[n] or null*/)
{
    using G = typename GlueOf<S, T>::type;
    constexpr bool FAST = sizeof(T) == 4;
    __shared__ double s_params[FD_MAX_TYPES * FD_NP_STAGED];
    __shared__ float s_pid_cfg[FD_NPID * FD_NPC];
    __shared__ G s_consts[FD_NC_STAGED];
    __shared__ G s_wps[FD_MAX_WAYPOINTS * FD_NWP];
    const LaneMap lm = lane_map(n);
    const int64_t i = lm.i;
    PidState st[FD_NPID];
    S x[FD_NX];
    int32_t idx = 0;
    int ty = 0;
    if (lm.on) {                                             // per-aircraft loads in flight during the staging below
#pragma unroll
        for (int k = 0; k < FD_NPID; ++k)
            st[k] = PidState{ pid_state[(k * FD_NPS + FD_PS_INTEGRAL) * n + i], pid_state[(k * FD_NPS + FD_PS_ERR_PREV) * n + i],
                              pid_state[(k * FD_NPS + FD_PS_DFILT) * n + i] };
#pragma unroll
        for (int k = 0; k < FD_NX; ++k) x[k] = xs[k * n + i];
        idx = wp_idx[i];
        ty = lane_type(type, i, n_types);
    }
    stage_params<FAST>(s_params, params, n_types);
    stage(s_pid_cfg, pid_cfg, FD_NPID * FD_NPC);
    stage_cascade_consts<G>(s_consts, consts);
    for (int k = threadIdx.x; k < n_wp * FD_NWP; k += blockDim.x) s_wps[k] = G(wps[k]);
    __syncthreads();
    if (!lm.on) return;

    const double* blk = s_params + ty * FD_NP_STAGED;
    Params<T> P; P.load(blk);
    Limits<S> Lm; Lm.load(blk);
    PidCfg cfg[FD_NPID];
#pragma unroll
    for (int k = 0; k < FD_NPID; ++k) cfg[k] = load_pid_cfg(s_pid_cfg, k);
    G Cr[FD_NC_STAGED];                                      // cascade constants in registers: read once, not once per control step
#pragma unroll
    for (int k = 0; k < FD_NC_STAGED; ++k) Cr[k] = s_consts[k];
    int32_t reached = 0;
    const bool restart = int(Cr[FD_C_ON_COMPLETE]) == 1;
    Surfaces<G> surf{ G(0), G(0), G(0), G(0) };

    if constexpr (FAST) {
        FastRK f;
        f.init(x);
        const float hdt = float(S(0.5) * dt), fdt = float(dt), dt6 = float(dt / S(6));
        for (int s = 0; s < n_steps; ++s) {
            if (idx < n_wp && waypoint_reached<G>(Cr, s_wps + idx * FD_NWP, f.x0)) { idx += 1; reached += 1; }   // mission.update
            if (idx >= n_wp) { if (restart) idx = 0; else break; }          // COMPLETE: freeze this aircraft
            const Derived<G> d = derived_fast(f);
            surf = waypoint_agent<G>(cfg, st, Cr, s_wps + idx * FD_NWP, f.x0, d, fdt);
            Controls<T> C;
            C.set(P, surf.elevator, surf.aileron, surf.rudder, surf.throttle);
            // controlled flight: an aircraft pushing against the rate clamp or flying sideways is an exception here, not a
            // standing share of the fleet -- the special cases stay behind their wave-level branches (STRAIGHT = false)
            rk4_fast_step<S, false>(P, Lm, C, x, f, hdt, fdt, dt6);
        }
    } else {
        for (int s = 0; s < n_steps; ++s) {
            if (idx < n_wp && waypoint_reached<S>(Cr, s_wps + idx * FD_NWP, x)) { idx += 1; reached += 1; }   // mission.update
            if (idx >= n_wp) { if (restart) idx = 0; else break; }          // COMPLETE: freeze this aircraft
            const Derived<S> d = derived<S>(x);
            surf = waypoint_agent<S>(cfg, st, Cr, s_wps + idx * FD_NWP, x, d, dt);
            Controls<T> C;
            C.set(P, surf.elevator, surf.aileron, surf.rudder, surf.throttle);
            rk4_substeps<S, T>(P, Lm, C, x, dt, 1);
        }
    }

#pragma unroll
    for (int k = 0; k < FD_NX; ++k) xs[k * n + i] = x[k];
#pragma unroll
    for (int k = 0; k < FD_NPID; ++k) {
        pid_state[(k * FD_NPS + FD_PS_INTEGRAL) * n + i] = st[k].integral;
        pid_state[(k * FD_NPS + FD_PS_ERR_PREV) * n + i] = st[k].err_prev;
        pid_state[(k * FD_NPS + FD_PS_DFILT) * n + i] = st[k].dfilt;
    }
    wp_idx[i] = idx;
    if (reached_total) reached_total[i] += reached;
    if (surf_out) {
        surf_out[FD_U_ELEVATOR * n + i] = S(surf.elevator); surf_out[FD_U_AILERON * n + i] = S(surf.aileron);
        surf_out[FD_U_RUDDER * n + i] = S(surf.rudder); surf_out[FD_U_THROTTLE * n + i] = S(surf.throttle);
    }
}

// ---------------------------------------------------------------------------------------------------------
// One cascade LEVEL commanded directly, per aircraft: n_steps x {agent.compute_action(command, state, dt) -> set_controls ->
// one RK4 of dt}, or with n_steps == 0 just compute_action (no physics).  This is how the reference's tests and examples
// drive RateAgent / AttitudeAgent / HSAAgent / WaypointAgent (controllers/*_agent.py; closed-loop helper
// tests/test_control_integration.py:34-74).  cmd rows by level:
//   FD_LEVEL_RATE     p, q, r [rad/s], throttle            FD_LEVEL_HSA       heading [rad], speed [m/s], altitude [m], -
//   FD_LEVEL_ATTITUDE roll, pitch, yaw (NaN = none), thr   FD_LEVEL_WAYPOINT  north, east, altitude, speed (NaN = keep)
// ---------------------------------------------------------------------------------------------------------
template <typename S, typename T>
__global__ void __launch_bounds__(FD_BLOCK, 1)
agent_step_kernel(int level, S* __restrict__ xs, float* __restrict__ pid_state /*[9*3][n]*/, const uint8_t* __restrict__ type,
                  const double* __restrict__ params, int n_types, const float* __restrict__ pid_cfg,
                  const double* __restrict__ consts, const S* __restrict__ cmd /*[4][n]*/, int64_t n, S dt, int n_steps,
                  S* __restrict__ surf_out /*[4][n]*/, int cfg_per_lane /*pid_cfg is [n][9][8]: one gain set per aircraft*/)
{
    using G = typename GlueOf<S, T>::type;
    constexpr bool FAST = sizeof(T) == 4;
    __shared__ double s_params[FD_MAX_TYPES * FD_NP_STAGED];
    __shared__ float s_pid_cfg[FD_NPID * FD_NPC];
    __shared__ G s_consts[FD_NC_STAGED];
    stage_params<FAST>(s_params, params, n_types);
    if (!cfg_per_lane) stage(s_pid_cfg, pid_cfg, FD_NPID * FD_NPC);
    stage_cascade_consts<G>(s_consts, consts);
    __syncthreads();
    const LaneMap lm = lane_map(n);
    const int64_t i = lm.i;
    if (!lm.on) return;
    const double* blk = s_params + lane_type(type, i, n_types) * FD_NP_STAGED;
    Params<T> P; P.load(blk);
    Limits<S> Lm; Lm.load(blk);
    PidCfg cfg[FD_NPID];
    PidState st[FD_NPID];
#pragma unroll
    for (int k = 0; k < FD_NPID; ++k) {
        cfg[k] = cfg_per_lane ? load_pid_cfg(pid_cfg + i * (FD_NPID * FD_NPC), k) : load_pid_cfg(s_pid_cfg, k);
        st[k] = PidState{ pid_state[(k * FD_NPS + FD_PS_INTEGRAL) * n + i], pid_state[(k * FD_NPS + FD_PS_ERR_PREV) * n + i],
                          pid_state[(k * FD_NPS + FD_PS_DFILT) * n + i] };
    }
    S x[FD_NX];
#pragma unroll
    for (int k = 0; k < FD_NX; ++k) x[k] = xs[k * n + i];
    const G c0 = G(cmd[i]), c1 = G(cmd[n + i]), c2 = G(cmd[2 * n + i]), c3 = G(cmd[3 * n + i]);
    Surfaces<G> surf{ G(0), G(0), G(0), G(0) };
    const int iters = n_steps > 0 ? n_steps : 1;
    const G gdt = G(dt);
    // one agent call on the glue-typed state `xg` with its derived scalars `dd` (a callable so both precisions share the switch)
    auto act = [&](const G (&xg)[FD_NX], auto&& derive) {
        if (level == FD_LEVEL_RATE) {
            surf = rate_agent<G>(cfg, st, s_consts, c0, c1, c2, c3, xg, gdt);
        } else if (level == FD_LEVEL_ATTITUDE) {
            const bool has_yaw = c2 == c2;
            surf = attitude_agent<G>(cfg, st, s_consts, c0, c1, has_yaw ? c2 : G(0), has_yaw, c3, xg, gdt);
        } else if (level == FD_LEVEL_HSA) {
            surf = hsa_agent<G>(cfg, st, s_consts, c0, c1, c2, xg, derive(), gdt);
        } else {
            const G wp[FD_NWP] = { c0, c1, c2, c3 };
            surf = waypoint_agent<G>(cfg, st, s_consts, wp, xg, derive(), gdt);
        }
    };
    if constexpr (FAST) {
        FastRK f;
        f.init(x);
        const float hdt = float(S(0.5) * dt), fdt = float(dt), dt6 = float(dt / S(6));
        for (int s = 0; s < iters; ++s) {
            act(f.x0, [&]() { return derived_fast(f); });
            if (n_steps > 0) {
                Controls<T> C;
                C.set(P, surf.elevator, surf.aileron, surf.rudder, surf.throttle);
                rk4_fast_step<S, false>(P, Lm, C, x, f, hdt, fdt, dt6);
            }
        }
    } else {
        for (int s = 0; s < iters; ++s) {
            act(x, [&]() { return derived<S>(x); });
            if (n_steps > 0) {
                Controls<T> C;
                C.set(P, surf.elevator, surf.aileron, surf.rudder, surf.throttle);
                rk4_substeps<S, T>(P, Lm, C, x, dt, 1);
            }
        }
    }
    if (n_steps > 0) {
#pragma unroll
        for (int k = 0; k < FD_NX; ++k) xs[k * n + i] = x[k];
    }
#pragma unroll
    for (int k = 0; k < FD_NPID; ++k) {
        pid_state[(k * FD_NPS + FD_PS_INTEGRAL) * n + i] = st[k].integral;
        pid_state[(k * FD_NPS + FD_PS_ERR_PREV) * n + i] = st[k].err_prev;
        pid_state[(k * FD_NPS + FD_PS_DFILT) * n + i] = st[k].dfilt;
    }
    if (surf_out) {
        surf_out[FD_U_ELEVATOR * n + i] = S(surf.elevator); surf_out[FD_U_AILERON * n + i] = S(surf.aileron);
        surf_out[FD_U_RUDDER * n + i] = S(surf.rudder); surf_out[FD_U_THROTTLE * n + i] = S(surf.throttle);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Hybrid cascade: PID outer loops over a learned (or PID) rate loop, one control step per launch
//   (controllers/attitude_agent.py:67,152 with `rate_agent = LearnedRateAgent(...)`, learned_rate_agent.py:128-198;
//    gui/simulation_worker_learned.py:51-118 switches the inner agent per aircraft)
// The policy runs between launches (its own kernels), so a launch is
//   1. apply: the surfaces of this control step -- the clipped policy action on learned lanes, the surfaces the rate PID
//      produced in the previous launch on PID lanes -- then one RK4 of dt;
//   2. the mission update and the outer agents on the new state, ending in a rate command + throttle;
//   3. PID lanes: the rate PID (its surfaces -> surf_out for the next launch); every lane: the policy observation.
// With actions == NULL only 2 and 3 run (x untouched): the priming call.
// ---------------------------------------------------------------------------------------------------------
// The stage under the attitude loop on a hybrid lane: records the rate command and throttle it is handed; runs the rate PID
// only where the lane is PID-controlled (its state advances only there).
template <typename G> struct HybridRateStage {
    bool pid;
    G p, q, r, thr;
    FD_DEV Surfaces<G> operator()(const PidCfg* cfg, PidState* st, const G* C, G p_cmd, G q_cmd, G r_cmd, G throttle,
                                  const G (&x)[FD_NX], G dt)
    {
        p = p_cmd; q = q_cmd; r = r_cmd; thr = clipv(throttle, G(0), G(1));      // rate_agent.py:122 / action bounds
        if (pid) return rate_agent<G>(cfg, st, C, p_cmd, q_cmd, r_cmd, throttle, x, dt);
        return Surfaces<G>{ G(0), G(0), G(0), thr };
    }
};

// (FD_BLOCK, 1) as the cascade: the same nine PID configurations / states, constants and integrator state in registers
template <typename S, typename T>
__global__ void __launch_bounds__(FD_BLOCK, 1)
hybrid_step_kernel(int level, S* __restrict__ xs, float* __restrict__ pid_state /*[9*3][n]*/, int32_t* __restrict__ wp_idx,
                   const uint8_t* __restrict__ type, const double* __restrict__ params, int n_types,
                   const float* __restrict__ pid_cfg, const double* __restrict__ consts, const S* __restrict__ cmd /*[4][n]*/,
                   const double* __restrict__ wps, int n_wp, const float* __restrict__ actions /*[n][4] or null*/,
                   const uint8_t* __restrict__ learned /*[n] or null = all*/, int throttle_src,
                   float* __restrict__ prev_action /*[n][4]*/, float* __restrict__ obs_out /*[n][18]*/,
                   float* __restrict__ rate_cmd_out /*[4][n] or null*/, S* __restrict__ surf_out /*[4][n]*/,
                   int32_t* __restrict__ reached_total, int64_t n, S dt)
{
    using G = typename GlueOf<S, T>::type;
    constexpr bool FAST = sizeof(T) == 4;
    __shared__ double s_params[FD_MAX_TYPES * FD_NP_STAGED];
    __shared__ float s_pid_cfg[FD_NPID * FD_NPC];
    __shared__ G s_consts[FD_NC_STAGED];
    __shared__ G s_wps[FD_MAX_WAYPOINTS * FD_NWP];
    const LaneMap lm = lane_map(n);
    const int64_t i = lm.i;
    const bool mission = wps != nullptr;
    PidState st[FD_NPID];
    S x[FD_NX];
    int32_t idx = 0;
    int ty = 0;
    bool is_pid = false;
    if (lm.on) {                                             // per-aircraft loads in flight during the staging below
#pragma unroll
        for (int k = 0; k < FD_NPID; ++k)
            st[k] = PidState{ pid_state[(k * FD_NPS + FD_PS_INTEGRAL) * n + i], pid_state[(k * FD_NPS + FD_PS_ERR_PREV) * n + i],
                              pid_state[(k * FD_NPS + FD_PS_DFILT) * n + i] };
#pragma unroll
        for (int k = 0; k < FD_NX; ++k) x[k] = xs[k * n + i];
        if (mission) idx = wp_idx[i];
        ty = lane_type(type, i, n_types);
        is_pid = learned ? learned[i] == 0 : false;
    }
    stage_params<FAST>(s_params, params, n_types);
    stage(s_pid_cfg, pid_cfg, FD_NPID * FD_NPC);
    stage_cascade_consts<G>(s_consts, consts);
    for (int k = threadIdx.x; k < n_wp * FD_NWP; k += blockDim.x) s_wps[k] = G(wps[k]);
    __syncthreads();
    if (!lm.on) return;

    const double* blk = s_params + ty * FD_NP_STAGED;
    Params<T> P; P.load(blk);
    Limits<S> Lm; Lm.load(blk);
    PidCfg cfg[FD_NPID];
#pragma unroll
    for (int k = 0; k < FD_NPID; ++k) cfg[k] = load_pid_cfg(s_pid_cfg, k);
    G Cr[FD_NC_STAGED];
#pragma unroll
    for (int k = 0; k < FD_NC_STAGED; ++k) Cr[k] = s_consts[k];
    const bool restart = int(Cr[FD_C_ON_COMPLETE]) == 1;
    // a mission the previous launch found complete (freeze): no physics, as the cascade's `break`
    bool frozen = mission && idx >= n_wp && !restart;
    float pa[FD_ACT_DIM];
#pragma unroll
    for (int k = 0; k < FD_ACT_DIM; ++k) pa[k] = prev_action[i * FD_ACT_DIM + k];
    const G gdt = G(dt);

    // ---- 1. apply ------------------------------------------------------------------------------------------------
    Surfaces<G> applied{ G(0), G(0), G(0), G(0) };
    if (actions) {
        const G thr_outer = G(surf_out[FD_U_THROTTLE * n + i]);
        if (!is_pid) {                                       // policy action [ail, elev, rud, thr], clipped to the action space
#pragma unroll
            for (int k = 0; k < FD_ACT_DIM; ++k) {
                const float a = actions[i * FD_ACT_DIM + k];
                pa[k] = clipv(a, k == 3 ? 0.0f : -1.0f, 1.0f);
                prev_action[i * FD_ACT_DIM + k] = pa[k];
            }
            applied = Surfaces<G>{ G(pa[1]), G(pa[0]), G(pa[2]),
                                   throttle_src == FD_HYBRID_THROTTLE_POLICY ? G(pa[3]) : thr_outer };
        } else {
            applied = Surfaces<G>{ G(surf_out[FD_U_ELEVATOR * n + i]), G(surf_out[FD_U_AILERON * n + i]),
                                   G(surf_out[FD_U_RUDDER * n + i]), thr_outer };
        }
        if (!frozen) {
            Controls<T> C;
            C.set(P, applied.elevator, applied.aileron, applied.rudder, applied.throttle);
            if constexpr (FAST) {
                FastRK f;
                f.init(x);
                rk4_fast_step<S, false>(P, Lm, C, x, f, float(S(0.5) * dt), float(dt), float(dt / S(6)));
            } else {
                rk4_substeps<S, T>(P, Lm, C, x, dt, 1);
            }
        }
    }

    // ---- 2. mission update + outer loops on the new state ---------------------------------------------------------
    // the fp32-evaluation glue reads a FastRK built afresh from the stored state -- exactly what a one-step cascade launch sees
    // (a K-step launch carries the incrementally rotated trigonometry across steps instead)
    HybridRateStage<G> inner;
    inner.pid = is_pid;
    inner.p = inner.q = inner.r = inner.thr = G(0);
    Surfaces<G> surf{ G(0), G(0), G(0), G(0) };
    int32_t reached = 0;
    auto outer = [&](const G (&xg)[FD_NX], auto&& derive) {
        if (mission) {
            if (idx < n_wp && waypoint_reached<G>(Cr, s_wps + idx * FD_NWP, xg)) { idx += 1; reached += 1; }   // mission.update
            if (idx >= n_wp) { if (restart) idx = 0; else frozen = true; }
            if (!frozen) surf = waypoint_agent<G>(cfg, st, Cr, s_wps + idx * FD_NWP, xg, derive(), gdt, inner);
            return;
        }
        const G c0 = G(cmd[i]), c1 = G(cmd[n + i]), c2 = G(cmd[2 * n + i]), c3 = G(cmd[3 * n + i]);
        if (level == FD_LEVEL_ATTITUDE) {
            const bool has_yaw = c2 == c2;
            surf = attitude_agent<G>(cfg, st, Cr, c0, c1, has_yaw ? c2 : G(0), has_yaw, c3, xg, gdt, inner);
        } else if (level == FD_LEVEL_HSA) {
            surf = hsa_agent<G>(cfg, st, Cr, c0, c1, c2, xg, derive(), gdt, inner);
        } else {
            const G wp[FD_NWP] = { c0, c1, c2, c3 };
            surf = waypoint_agent<G>(cfg, st, Cr, wp, xg, derive(), gdt, inner);
        }
    };
    if constexpr (FAST) {
        FastRK f;
        f.init(x);
        outer(f.x0, [&]() { return derived_fast(f); });
    } else {
        outer(x, [&]() { return derived<S>(x); });
    }

    // ---- 3. inner loop outputs ---------------------------------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < FD_NX; ++k) if (actions) xs[k * n + i] = x[k];
#pragma unroll
    for (int k = 0; k < FD_NPID; ++k) {
        pid_state[(k * FD_NPS + FD_PS_INTEGRAL) * n + i] = st[k].integral;
        pid_state[(k * FD_NPS + FD_PS_ERR_PREV) * n + i] = st[k].err_prev;
        pid_state[(k * FD_NPS + FD_PS_DFILT) * n + i] = st[k].dfilt;
    }
    if (mission) {
        wp_idx[i] = idx;
        if (reached_total) reached_total[i] += reached;
    }
    // PID lanes: the surfaces the next launch applies (zero when frozen, as the cascade's surf_out).  Learned lanes: the
    // outer-loop throttle (read back by the next launch under FD_HYBRID_THROTTLE_OUTER) and the surfaces applied here.
    if (is_pid) {
        surf_out[FD_U_ELEVATOR * n + i] = S(surf.elevator); surf_out[FD_U_AILERON * n + i] = S(surf.aileron);
        surf_out[FD_U_RUDDER * n + i] = S(surf.rudder);
    } else if (actions) {
        surf_out[FD_U_ELEVATOR * n + i] = S(applied.elevator); surf_out[FD_U_AILERON * n + i] = S(applied.aileron);
        surf_out[FD_U_RUDDER * n + i] = S(applied.rudder);
    }
    surf_out[FD_U_THROTTLE * n + i] = S(surf.throttle);
    // the rate command handed to the inner loop, narrowed to fp32: what rate_cmd_out reports and what the observation is built
    // from, so that a host composition fed rate_cmd_out assembles the same observation (learned_rate_agent.py:152-178)
    const float rc[4] = { float(inner.p), float(inner.q), float(inner.r), float(inner.thr) };
    if (rate_cmd_out) {
#pragma unroll
        for (int k = 0; k < 4; ++k) rate_cmd_out[k * n + i] = rc[k];
    }
    {
#pragma clang fp contract(off)
        // clip and differences in the state's precision, then narrowed (rate_env.py:374-408)
        float* o = obs_out + i * FD_OBS_DIM;
        const double mr[3] = { consts[FD_C_MAX_ROLL_RATE], consts[FD_C_MAX_PITCH_RATE], consts[FD_C_MAX_YAW_RATE] };
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const S c = clipv(S(rc[k]), -S(mr[k]), S(mr[k]));
            o[k] = float(x[9 + k]);
            o[3 + k] = float(c);
            o[6 + k] = float(c - x[9 + k]);
        }
        o[9] = float(M<S>::sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]));
        o[10] = float(-x[2]);
        o[11] = float(x[6]); o[12] = float(x[7]); o[13] = float(x[8]);
#pragma unroll
        for (int k = 0; k < FD_ACT_DIM; ++k) o[14 + k] = pa[k];
    }
}

// ---------------------------------------------------------------------------------------------------------
// K3+K4: RateControlEnv.step for a whole vec-env, with done compaction and in-kernel auto-reset
// ---------------------------------------------------------------------------------------------------------
template <typename G> struct EnvConsts {
    G dt, mr0, mr1, mr2, scale;     // separate scalars: an indexed array here ends up in scratch
    int max_steps, cmd_type, n_sub;
    int settle_steps;               // consecutive settled steps at which the reference's accumulated timer reaches 0.2 s
    // arithmetic select: a ?: chain over struct fields is turned back into an indexed (scratch) load by the compiler
    __device__ __forceinline__ G max_rate(int ax) const { return mr0 * G(ax == 0) + mr1 * G(ax == 1) + mr2 * G(ax == 2); }
};

// `sched`: the four schedule words are live only for ramp / sine commands (rate_env.py:342-372); step and random-walk
// fleets neither read nor write them (64 B per env per step at fp64) -- they stay 0, which is what reset leaves there
template <typename G>
__device__ __forceinline__ void env_load(EnvState<G>& e, const G* __restrict__ es, int64_t n, int64_t i, bool sched = true)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e.cmd[k] = es[(FD_E_CMD_P + k) * n + i];
        e.prev_err[k] = es[(FD_E_PERR_P + k) * n + i];
        e.sign_changes[k] = es[(FD_E_SIGN_P + k) * n + i];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        e.prev_action[k] = es[(FD_E_PREV_AIL + k) * n + i];
        e.sched[k] = sched ? es[(FD_E_SCHED0 + k) * n + i] : G(0);
    }
    e.settle_timer = es[FD_E_SETTLE_TIMER * n + i]; e.is_settled = es[FD_E_IS_SETTLED * n + i];
    e.time = es[FD_E_TIME * n + i]; e.ep_return = es[FD_E_EP_RETURN * n + i];
}
template <typename G>
__device__ __forceinline__ void env_store(const EnvState<G>& e, G* __restrict__ es, int64_t n, int64_t i, bool sched = true)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        es[(FD_E_CMD_P + k) * n + i] = e.cmd[k];
        es[(FD_E_PERR_P + k) * n + i] = e.prev_err[k];
        es[(FD_E_SIGN_P + k) * n + i] = e.sign_changes[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        es[(FD_E_PREV_AIL + k) * n + i] = e.prev_action[k];
        if (sched) es[(FD_E_SCHED0 + k) * n + i] = e.sched[k];
    }
    es[FD_E_SETTLE_TIMER * n + i] = e.settle_timer; es[FD_E_IS_SETTLED * n + i] = e.is_settled;
    es[FD_E_TIME * n + i] = e.time; es[FD_E_EP_RETURN * n + i] = e.ep_return;
}

// one reset record drawn on the device (throughput mode): same distributions as
// learned_controllers/data/generators.py:47-72,74-125,190-214 and rate_env.py:306, Philox instead of MT19937
template <typename G>
__device__ __forceinline__ void device_reset_record(uint64_t seed, uint32_t env, uint32_t episode,
                                                    const EnvConsts<G>& ec, G (&rec)[FD_NR])
{
    Philox ph;
    uint32_t r0[4], r1[4], r2[4], r3[4];
    ph.block(seed, env, episode, 0u, FD_PHX_RESET + 0, r0);
    ph.block(seed, env, episode, 0u, FD_PHX_RESET + 1, r1);
    ph.block(seed, env, episode, 0u, FD_PHX_RESET + 2, r2);
    ph.block(seed, env, episode, 0u, FD_PHX_RESET + 3, r3);
    const float d15 = 0.26179938779914943f;     // radians(15)
    rec[FD_R_AIRSPEED] = G(15.0f + 15.0f * u01(r0[0]));
    rec[FD_R_ALTITUDE] = G(50.0f + 150.0f * u01(r0[1]));
    rec[FD_R_ROLL] = G(-d15 + 2.0f * d15 * u01(r0[2]));
    rec[FD_R_PITCH] = G(-d15 + 2.0f * d15 * u01(r0[3]));
    rec[FD_R_YAW] = G(6.283185307179586f * u01(r1[0]));
    rec[FD_R_P] = G(-0.1f + 0.2f * u01(r1[1]));
    rec[FD_R_Q] = G(-0.1f + 0.2f * u01(r1[2]));
    rec[FD_R_R] = G(-0.1f + 0.2f * u01(r1[3]));
    rec[FD_R_CMD0] = rec[FD_R_CMD1] = rec[FD_R_CMD2] = rec[FD_R_CMD3] = G(0);
    if (ec.cmd_type == FD_CMD_RANDOM_WALK) return;
    const bool sine = ec.cmd_type == FD_CMD_SINE;
    int k = sine ? 1 + int(u01(r2[0]) * 2.0f) : 1 + int(u01(r2[0]) * 3.0f);          // number of active axes
    k = k > 3 ? 3 : k;
    // Which axes are active: a random permutation (first, second, third) of the three axes, first k of it active.
    // Everything below is straight-line scalar selects with STATIC array indices: a run-time index into a private
    // array (or a ?: chain over array elements, which the compiler folds back into one) is mis-compiled / spilled.
    const int perm = int(u01(r2[1]) * 6.0f) % 6;
    const int first = perm >> 1;
    const int o1 = first == 2 ? 0 : first + 1, o2 = first == 0 ? 2 : first - 1;
    const int second = (perm & 1) ? o2 : o1;
    const float m0 = u01(r3[0]), m1 = u01(r3[1]), m2 = u01(r3[2]);
    const G mrs[3] = { ec.mr0, ec.mr1, ec.mr2 };
    G vals[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {                                  // a is a compile-time constant after unrolling
        const int pos = (a == first) ? 0 : ((a == second) ? 1 : 2);
        const float um = pos == 0 ? m0 : (pos == 1 ? m1 : m2);
        float mag = (0.3f + 0.7f * um) * float(ec.scale);
        if (sine) mag *= 0.5f;
        const float sgn = (!sine && ((r2[2] >> pos) & 1u)) ? -1.0f : 1.0f;
        vals[a] = (pos < k) ? G(sgn * mag) * mrs[a] : G(0);
    }
    rec[FD_R_CMD0] = vals[0]; rec[FD_R_CMD1] = vals[1]; rec[FD_R_CMD2] = vals[2];
    if (sine) rec[FD_R_CMD3] = G(0.1f + 1.9f * u01(r2[3]));
}

// RateControlEnv.reset body (rate_env.py:170-204) from one record
template <typename G, typename E>
__device__ __forceinline__ void env_apply_reset(const G (&rec)[FD_NR], int cmd_type, G (&x)[FD_NX], EnvState<E>& e)
{
#pragma unroll
    for (int k = 0; k < FD_NX; ++k) x[k] = G(0);
    x[2] = -rec[FD_R_ALTITUDE]; x[3] = rec[FD_R_AIRSPEED];
    x[6] = rec[FD_R_ROLL]; x[7] = rec[FD_R_PITCH]; x[8] = rec[FD_R_YAW];
    x[9] = rec[FD_R_P]; x[10] = rec[FD_R_Q]; x[11] = rec[FD_R_R];
#pragma unroll
    for (int k = 0; k < 3; ++k) { e.cmd[k] = E(0); e.prev_err[k] = E(0); e.sign_changes[k] = E(0); e.prev_action[k] = E(0); }
#pragma unroll
    for (int k = 0; k < 4; ++k) e.sched[k] = E(0);
    e.prev_action[3] = E(0.5);                                                   // rate_env.py:193
    if (cmd_type == FD_CMD_STEP) {
        e.cmd[0] = E(rec[FD_R_CMD0]); e.cmd[1] = E(rec[FD_R_CMD1]); e.cmd[2] = E(rec[FD_R_CMD2]);
    } else if (cmd_type == FD_CMD_RAMP || cmd_type == FD_CMD_SINE) {
        e.sched[0] = E(rec[FD_R_CMD0]); e.sched[1] = E(rec[FD_R_CMD1]); e.sched[2] = E(rec[FD_R_CMD2]); e.sched[3] = E(rec[FD_R_CMD3]);
    }
    e.settle_timer = E(0); e.is_settled = E(0); e.time = E(0); e.ep_return = E(0);
}

// PREP: EC is the env-constant section of a launch image (FD_EC_* words followed by the derived FD_ECD_* ones,
// fdyn_rate_env_image): the two derived counts are read, not recomputed by every wave of every launch.
template <typename G, bool PREP = false>
__device__ __forceinline__ void load_env_consts(const double* __restrict__ EC, EnvConsts<G>& ec)
{
    ec.dt = G(EC[FD_EC_DT]);
    if constexpr (!PREP) {
        ec.max_steps = int(EC[FD_EC_MAX_STEPS]);
        ec.cmd_type = int(EC[FD_EC_CMD_TYPE]);
    }
    ec.scale = G(EC[FD_EC_DIFFICULTY_SCALE]);
    ec.mr0 = G(EC[FD_EC_MAX_RATE_P]); ec.mr1 = G(EC[FD_EC_MAX_RATE_Q]); ec.mr2 = G(EC[FD_EC_MAX_RATE_R]);
    if constexpr (PREP) {
        const int32_t* __restrict__ ic = reinterpret_cast<const int32_t*>(EC + FD_ECD_INTS);
        ec.max_steps = ic[0]; ec.cmd_type = ic[1]; ec.n_sub = ic[2]; ec.settle_steps = ic[3];
        return;
    }
    const double r = EC[FD_EC_DT] / EC[FD_EC_DT_PHYSICS];                       // simulation_backend.py:95
    const long ns = long(r);
    ec.n_sub = ns < 1 ? 1 : int(ns);
    // rewards.py:205-209: `timer += dt; if timer >= 0.2` in fp64 -- 0.02 x 10 accumulates to 0.19999999999999998, so the bonus
    // starts at the 11th settled step.  The fp32 env words carry the step COUNT; this is the count the sum first reaches 0.2 at.
    const double dts = EC[FD_EC_DT];
    int k = 0;
    if (dts >= 1.0e-3) { double t = 0.0; while (t < 0.2 && k < 256) { t += dts; ++k; } }
    else k = int(0.2 / dts) + 1;
    ec.settle_steps = k;
}

template <typename G>
__device__ __forceinline__ void fetch_reset_record(const double* __restrict__ pool, int pool_depth, uint64_t seed,
                                                   int64_t i, int32_t episode, const EnvConsts<G>& ec, G (&rec)[FD_NR])
{
    if (pool) {
        const double* r = pool + (i * pool_depth + (episode % pool_depth)) * FD_NR;
#pragma unroll
        for (int k = 0; k < FD_NR; ++k) rec[k] = G(r[k]);
        // the record is complete when this branch ends: with a load still in flight at the join with the drawn record's path,
        // every later reader of rec[] waits for ALL outstanding memory operations, whichever path the wave took
#pragma unroll
        for (int k = 0; k < FD_NR; ++k) asm volatile("" : "+v"(rec[k]));
    } else {
        device_reset_record<G>(seed, uint32_t(i), uint32_t(episode), ec, rec);
    }
}

// coalesced write-out of a wave's 64 x 18 observation tile through LDS (row stride 19 words: conflict-free)
// WT: the store policy (put / put16_through, fdyn_fleet.hpp), on both paths
template <bool WT = false>
__device__ __forceinline__ void store_obs_tile(float* tile /*[64*19]*/, const float (&o)[FD_OBS_DIM], int lane,
                                               float* __restrict__ obs_out, int64_t wave_first, int64_t n)
{
    int64_t valid = n - wave_first;
    valid = valid < 0 ? 0 : (valid < FD_WAVE ? valid : FD_WAVE);
    float* dst = obs_out + wave_first * FD_OBS_DIM;
    static_assert(FD_OBS_DIM == 18 && FD_WAVE == 64, "the full-wave path below moves 64 x 18 floats as 288 float4");
    if (valid == FD_WAVE && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        // a full wave's tile is 4608 contiguous bytes of obs_out: rows go to LDS unpadded (nine 8-byte writes per lane) and
        // leave as 4.5 rounds of 16-byte loads / stores -- 9 + 5 + 5 memory instructions with no index arithmetic instead of
        // 18 + 18 + 18 with a division by 18 each (2.8 k of a wave's 96 k cycles per env step, scratch/phase_stamps.py)
        float2* row = reinterpret_cast<float2*>(tile + lane * FD_OBS_DIM);
#pragma unroll
        for (int k = 0; k < FD_OBS_DIM / 2; ++k) row[k] = make_float2(o[2 * k], o[2 * k + 1]);
        __builtin_amdgcn_wave_barrier();
        const float4* t4 = reinterpret_cast<const float4*>(tile);
        if constexpr (WT) {
            constexpr uint32_t TILE_BYTES = FD_WAVE * FD_OBS_DIM * sizeof(float);
#pragma unroll
            for (int j = 0; j < 4; ++j) put16_through(dst, TILE_BYTES, uint32_t(j * FD_WAVE + lane) * 16u, t4[j * FD_WAVE + lane]);
            if (lane < FD_WAVE / 2) put16_through(dst, TILE_BYTES, uint32_t(4 * FD_WAVE + lane) * 16u, t4[4 * FD_WAVE + lane]);
        } else {
            float4* d4 = reinterpret_cast<float4*>(dst);
#pragma unroll
            for (int j = 0; j < 4; ++j) d4[j * FD_WAVE + lane] = t4[j * FD_WAVE + lane];
            if (lane < FD_WAVE / 2) d4[4 * FD_WAVE + lane] = t4[4 * FD_WAVE + lane];
        }
        __builtin_amdgcn_wave_barrier();
        return;
    }
#pragma unroll
    for (int k = 0; k < FD_OBS_DIM; ++k) tile[lane * (FD_OBS_DIM + 1) + k] = o[k];
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < FD_OBS_DIM; ++k) {
        const int flat = k * FD_WAVE + lane;
        const int row = flat / FD_OBS_DIM, col = flat - row * FD_OBS_DIM;
        if (row < valid) FD_PUT(WT, dst[flat], tile[row * (FD_OBS_DIM + 1) + col]);
    }
    __builtin_amdgcn_wave_barrier();
}

// ---- domain randomisation (the _dr entry points; DESIGN.md "Domain randomisation") ----------------------------------------
// the env kernels take the randomisation arguments as a trailing pack: empty for the plain env, (dr, dr_consts) for the _dr one
template <typename S> __device__ __forceinline__ void dr_unpack(S*& dr, const double*& drc, S* d, const double* c) { dr = d; drc = c; }
// three standard normals from one Philox block (Box-Muller on its four words; fp32 transcendentals: statistical use only)
__device__ __forceinline__ void dr_normals3(uint64_t seed, uint32_t env, uint32_t episode, uint32_t step, uint32_t word, float (&z)[3])
{
    Philox ph; uint32_t r[4];
    ph.block(seed, env, episode, step, word, r);
    const float m0 = fast::sqrt(-2.0f * __logf(u01(r[0]))), m1 = fast::sqrt(-2.0f * __logf(u01(r[2])));
    float s0, c0, s1, c1;
    fast::sincos(6.283185307179586f * u01(r[1]), s0, c0);
    fast::sincos(6.283185307179586f * u01(r[3]), s1, c1);
    z[0] = m0 * c0; z[1] = m0 * s0; z[2] = m1 * c1;
}
// air-relative body velocity of the stored state under the air-mass velocity W (NED), in the glue type A
template <typename A, typename S>
__device__ __forceinline__ void air_velocity(const S (&x)[FD_NX], const S (&W)[3], A& ua, A& va, A& wa)
{
    A sp, cp, st, ct, sy, cy, bu, bv, bw;
    M<A>::sincos(A(x[6]), sp, cp); M<A>::sincos(A(x[7]), st, ct); M<A>::sincos(A(x[8]), sy, cy);
    body_wind<A>(sp, cp, st, ct, sy, cy, Wind<A>{ A(W[0]), A(W[1]), A(W[2]) }, bu, bv, bw);
    ua = A(x[3]) - bu; va = A(x[4]) - bv; wa = A(x[5]) - bw;
}
template <typename A, typename S>
__device__ __forceinline__ A air_speed(const S (&x)[FD_NX], const S (&W)[3])
{
    A ua, va, wa;
    air_velocity<A, S>(x, W, ua, va, wa);
    return M<A>::sqrt(ua * ua + va * va + wa * wa);
}
// The randomisation part of a reset, after env_apply_reset has set x from the record: with FD_DC_REDRAW set, draw every row
// from its range (Philox words FD_PHX_DR_RESET.. and FD_PHX_DR_GUST0, keyed like the record) and store it; otherwise read the
// wind and gust the host left.  Then make the record's airspeed air-relative: v = (V0, 0, 0) + R^T (W + g0).  Returns W + g0.
template <typename S>
__device__ __forceinline__ void dr_reset(uint64_t seed, uint32_t env, uint32_t episode, const double* __restrict__ drc, double dt,
                                         S* __restrict__ dr, int64_t n, int64_t i, S (&x)[FD_NX], S (&wair)[3])
{
    if (drc[FD_DC_REDRAW] != 0.0) {
        Philox ph;
        uint32_t r0[4], r1[4], r2[4];
        ph.block(seed, env, episode, 0u, FD_PHX_DR_RESET, r0);
        ph.block(seed, env, episode, 0u, FD_PHX_DR_RESET + 1, r1);
        ph.block(seed, env, episode, 0u, FD_PHX_DR_RESET + 2, r2);
        const uint32_t u[10] = { r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3], r2[0], r2[1] };
        double v[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) {                    // range k = words 2k, 2k+1 of dr_consts; lo == hi gives lo exactly
            const double lo = drc[2 * k], hi = drc[2 * k + 1];
            v[k] = lo + (hi - lo) * double(u01(u[k]));
        }
        float sd, cd;
        fast::sincos(float(v[1]), sd, cd);                // direction: an fp32 angle is plenty for a random draw
        float z[3];
        dr_normals3(seed, env, episode, 0u, FD_PHX_DR_GUST0, z);
        const double V0 = double(x[3]);                   // the record's airspeed (x is still the still-air IC here)
        const double sigma = v[3] * V0;                   // intensity x reset airspeed
        const double a = exp(-dt * V0 / v[4]);            // first-order Gauss-Markov gust over one env step
        const S row[FD_NDR] = { S(v[0] * double(cd)), S(v[0] * double(sd)), S(v[2]),
                                S(sigma * double(z[0])), S(sigma * double(z[1])), S(sigma * double(z[2])),
                                S(a), S(sigma * sqrt(1.0 - a * a)),
                                S(v[5]), S(v[6]), S(v[7]), S(v[8]), S(v[9]) };
#pragma unroll
        for (int k = 0; k < FD_NDR; ++k) dr[k * n + i] = row[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) wair[k] = row[FD_DR_WIND_N + k] + row[FD_DR_GUST_N + k];
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) wair[k] = dr[(FD_DR_WIND_N + k) * n + i] + dr[(FD_DR_GUST_N + k) * n + i];
    }
    S sp, cp, st, ct, sy, cy, bu, bv, bw;
    M<S>::sincos(x[6], sp, cp); M<S>::sincos(x[7], st, ct); M<S>::sincos(x[8], sy, cy);
    body_wind<S>(sp, cp, st, ct, sy, cy, Wind<S>{ wair[0], wair[1], wair[2] }, bu, bv, bw);
    x[3] = x[3] + bu; x[4] = x[4] + bv; x[5] = x[5] + bw;
}

// DRA = {} : the plain env ; DRA = {S*, const double*} : the _dr entry points (dr rows, dr_consts).  A trailing parameter pack,
// so that the plain instantiation keeps its argument list, kernarg layout and instructions.
template <typename S, typename E, typename... DRA>
__global__ void __launch_bounds__(FD_BLOCK)
rate_env_reset_kernel(S* __restrict__ xs, E* __restrict__ es, int32_t* __restrict__ eis, float* __restrict__ pid_state,
                      const uint8_t* __restrict__ mask, const double* __restrict__ EC, const double* __restrict__ pool,
                      int pool_depth, uint64_t seed, float* __restrict__ obs_out, int64_t n, DRA... dra)
{
    __shared__ __attribute__((aligned(16))) float s_tile[FD_BLOCK / FD_WAVE][FD_WAVE * (FD_OBS_DIM + 1)];
    constexpr bool DR = sizeof...(DRA) != 0;
    S* dr = nullptr;
    const double* drc = nullptr;
    if constexpr (DR) dr_unpack(dr, drc, dra...);
    const LaneMap lm = lane_map(n);
    const int64_t i = lm.i;
    const int lane = lm.lane, wave = threadIdx.x / FD_WAVE;
    const bool active = lm.on;
    EnvConsts<S> ec;
    load_env_consts<S>(EC, ec);
    S x[FD_NX];
    EnvState<E> e;
    float o[FD_OBS_DIM];
#pragma unroll
    for (int k = 0; k < FD_OBS_DIM; ++k) o[k] = 0.0f;
    if (active) {
        const bool doit = mask ? mask[i] != 0 : true;
        S wair[3];
        if (doit) {
            const int32_t episode = eis[FD_EI_EPISODE * n + i];
            S rec[FD_NR];
            fetch_reset_record<S>(pool, pool_depth, seed, i, episode, ec, rec);
            env_apply_reset<S, E>(rec, ec.cmd_type, x, e);
            if constexpr (DR) dr_reset<S>(seed, uint32_t(i), uint32_t(episode), drc, EC[FD_EC_DT], dr, n, i, x, wair);
#pragma unroll
            for (int k = 0; k < FD_NX; ++k) xs[k * n + i] = x[k];
            env_store<E>(e, es, n, i);
            eis[FD_EI_STEP * n + i] = 0;
            eis[FD_EI_EPISODE * n + i] = episode + 1;
            if (pid_state) for (int k = 0; k < 3 * FD_NPS; ++k) pid_state[k * n + i] = 0.0f;
        } else {
#pragma unroll
            for (int k = 0; k < FD_NX; ++k) x[k] = xs[k * n + i];
            env_load<E>(e, es, n, i);
            if constexpr (DR) {
#pragma unroll
                for (int k = 0; k < 3; ++k) wair[k] = dr[(FD_DR_WIND_N + k) * n + i] + dr[(FD_DR_GUST_N + k) * n + i];
            }
        }
        S airspeed, altitude;
        airspeed_altitude<S>(x, airspeed, altitude);
        if constexpr (DR) airspeed = air_speed<S, S>(x, wair);                   // the air-relative airspeed
        env_observation<S, S, E>(x, e, airspeed, altitude, o);
    }
    store_obs_tile(s_tile[wave], o, lane, obs_out, lm.wave_first, n);
}

#ifdef FD_PHASE_STAMPS
// timing experiment (scratch/phase_stamps.py; never in the shipped build): shader-clock stamps of wave 0 of every workgroup at
// five points of the env step -> where the 22 % of wave cycles that rocprofv3 reports as waiting are spent
__device__ unsigned long long fdyn_stamps[4096 * 8];
#define FD_STAMP(K) if (threadIdx.x == 0 && blockIdx.x < 4096) fdyn_stamps[blockIdx.x * 8 + (K)] = __builtin_readcyclecounter();
#define FD_STAMP_REAL(K) if (threadIdx.x == 0 && blockIdx.x < 4096) fdyn_stamps[blockIdx.x * 8 + (K)] = wall_clock64();   /* 100 MHz, chip-wide */
extern "C" int fdyn_debug_read_stamps(unsigned long long* out, int count)
{
    return int(hipMemcpyFromSymbol(out, HIP_SYMBOL(fdyn_stamps), sizeof(unsigned long long) * size_t(count)));
}
extern "C" int fdyn_debug_read_counts(unsigned* out, int count, int clear)
{
    int rc = int(hipMemcpyFromSymbol(out, HIP_SYMBOL(fdyn_dbg_cnt), sizeof(unsigned) * size_t(count)));
    if (clear && rc == 0) {
        void* p = nullptr;
        rc = int(hipGetSymbolAddress(&p, HIP_SYMBOL(fdyn_dbg_cnt)));
        if (rc == 0) rc = int(hipMemset(p, 0, sizeof(unsigned) * 4096 * 8));
    }
    return rc;
}
#else
#define FD_STAMP(K)
#define FD_STAMP_REAL(K)
#endif

// OCC2: cap the registers at 256 so that two waves fit per SIMD.  At exactly one wave per SIMD (65 536 envs on 256 CUs) the
// uncapped allocation (258 VGPRs) is 4 % faster; past that the second wave hides the first one's issue gaps
// (1 Mi envs: 1.16e9 -> 1.56e9 env-steps/s).  The launcher picks by batch size; the arithmetic is the same.
// DR = true: the _dr entry points -- wind + gust in the aerodynamics, per-env parameter scales, the gust update and the
// randomising resets (DESIGN.md "Domain randomisation").  DR = false is the plain env and compiles to its former instructions.
// PREP = true: the _img entry points -- `params` is the staged block section of a prepared launch image ([n_types][FD_NP_STAGED],
// derived words included) and `EC` its env-constant section; the kernel copies and reads, it derives nothing.
template <typename S, typename T, bool OCC2, bool PREP, typename... DRA>
__global__ void __launch_bounds__(FD_BLOCK, OCC2 ? 2 : 1)
rate_env_step_kernel(S* __restrict__ xs, typename EnvOf<S, T>::type* __restrict__ es, int32_t* __restrict__ eis,
                     const uint8_t* __restrict__ type, const double* __restrict__ params, int n_types,
                     const double* __restrict__ EC,
                     const float* __restrict__ actions /*[n][4] or null => in-kernel rate PID*/,
                     float* __restrict__ pid_state /*[3*3][n], PID mode*/, const float* __restrict__ pid_cfg /*[9][8]*/,
                     const double* __restrict__ casc_consts /*[FD_NC], PID mode*/, float* __restrict__ actions_out,
                     const S* __restrict__ rw_delta /*[3][n] or null*/,
                     const double* __restrict__ pool, int pool_depth, uint64_t seed, int auto_reset, float residual_scale,
                     float* __restrict__ obs_out /*[n][18]*/, float* __restrict__ reward_f32, S* __restrict__ reward_full,
                     uint8_t* __restrict__ terminated, uint8_t* __restrict__ truncated,
                     int32_t* __restrict__ ev_count, int32_t* __restrict__ ev_count_next, int32_t* __restrict__ ev_int,
                     float* __restrict__ ev_flt, int ev_cap, int64_t n, DRA... dra)
{
    constexpr bool DR = sizeof...(DRA) != 0;
    // The image entry points at one wave per SIMD write the state, the fp64 reward, the observation tile, the PID state and
    // actions_out THROUGH L2 (FD_PUT / put16_through, fdyn_fleet.hpp): 11 of the 17 MB a launch stores, all of it issued in a
    // wave's last 2 us, otherwise sit dirty in L2 until the launch's closing release writes them back with every SIMD idle.
    // The env words, the two integer words and the fp32 reward stay plain -- 4-byte write-through stores are the expensive
    // kind, and with them the step measured no faster (profiles/env_store_policy_measured.md) -- and so do the flags, the
    // event records and the counters (131 KB in all).  The plain entry points and the register-capped build (whose output
    // exceeds L2 anyway) keep plain stores and their text.
    constexpr bool WT = PREP && !OCC2;
    S* dr = nullptr;
    const double* drc = nullptr;
    if constexpr (DR) dr_unpack(dr, drc, dra...);
    __shared__ double s_params[FD_MAX_TYPES * FD_NP_STAGED];
    __shared__ __attribute__((aligned(16))) float s_tile[FD_BLOCK / FD_WAVE][FD_WAVE * (FD_OBS_DIM + 1)];
    __shared__ float s_pid_cfg[3 * FD_NPC];
    __shared__ S s_consts[FD_NC];
    FD_STAMP(0)
    FD_STAMP_REAL(7)
    const LaneMap lm = lane_map(n);
    const int64_t i = lm.i;
    const int lane = lm.lane, wave = threadIdx.x / FD_WAVE;
    const bool active = lm.on;
    EnvConsts<S> ec;
    load_env_consts<S, PREP>(EC, ec);
    const bool uses_sched = ec.cmd_type == FD_CMD_RAMP || ec.cmd_type == FD_CMD_SINE;
    // the benched build (mixed precision, one wave per SIMD, prepared image, still air) holds the sub-step loop twice: the general
    // one and the one without dynamics_fast's rare block, chosen per wave from the image's FD_ECD_SMALL_STEPS word
    constexpr bool TWO_LOOPS = PREP && !OCC2 && !DR && sizeof(S) == 8 && sizeof(T) == 4;
    bool small_steps = false;
    if constexpr (TWO_LOOPS) small_steps = EC[FD_ECD_SMALL_STEPS] != 0.0;
    // actions == null: the fused rate-PID demonstrator drives the env.  residual_scale > 0 (with actions AND pid state):
    // ResidualRateControlEnv -- action = clip(PID + scale * residual) (residual_rate_env.py:99-157).
    const bool residual_mode = actions != nullptr && residual_scale > 0.0f && pid_state != nullptr;
    const bool pid_mode = actions == nullptr || residual_mode;

    // ---- every per-env global load is issued HERE, before the parameter staging and its barrier: the HBM round trip of
    // the state overlaps the staging chain instead of following it
    using E = typename EnvOf<S, T>::type;
    S x[FD_NX];
    EnvState<E> e;
    int32_t step = 0, episode = 0;
    int ty = 0;
    float4 av = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // The reset record of an env that ends in this launch depends only on (seed, env, episode): with device sampling it is drawn
    // HERE, while the state loads are in flight -- at one wave per SIMD every wave of the launch loads at the same moment, the
    // 13 MB burst takes ~7 k cycles and the wave has nothing else to do, whereas at the end of the step the four Philox blocks
    // (80 quarter-rate 64-bit multiplies, ~2.5 k cycles) were paid by three waves in four, the slowest ones included.  The
    // episode counter is therefore loaded FIRST (loads return in order).  The register-capped build keeps the lazy draw: its
    // neighbour wave hides it, and 24 more live registers would spill.
    // Order of the requests = order of arrival: the parameter words (the barrier below waits for them), the episode counter (the
    // reset record), what the FIRST dynamics evaluation reads (velocities, angles, rates, the action), and only then the position
    // (first touched by the accumulate at the end of sub-step 1) and the env words (touched after the 20 sub-steps) -- the second
    // half of the burst lands under the first sub-step instead of in front of it.
    S rec_pre[FD_NR];
    S wair[3] = { S(0), S(0), S(0) }, dsc[5] = { S(1), S(1), S(1), S(1), S(1) };   // DR: air-mass velocity W + g, parameter scales
    const bool pre_drawn = !OCC2 && pool == nullptr && auto_reset != 0;
    // (fp32-evaluation builds only: in the fp64 build the split left a dead 20-byte private segment in the kernel descriptor --
    // never accessed, but a scratch set-up per launch -- and that build is the parity reference, not the benched one)
    constexpr bool EARLY_PARAMS = sizeof(T) == 4;
    StagedParamWords spw = { 0.0, 0.0, 1.0 };
    if constexpr (EARLY_PARAMS) spw = PREP ? stage_image_early(params, n_types) : stage_params_early(params, n_types);
    if (active) {
        episode = eis[FD_EI_EPISODE * n + i];
#pragma unroll
        for (int k = 3; k < FD_NX; ++k) x[k] = xs[k * n + i];
        if (actions) av = reinterpret_cast<const float4*>(actions)[i];
        ty = lane_type(type, i, n_types);
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = xs[k * n + i];
        step = eis[FD_EI_STEP * n + i];
        env_load<E>(e, es, n, i, uses_sched);
        if (pre_drawn) device_reset_record<S>(seed, uint32_t(i), uint32_t(episode), ec, rec_pre);
        if constexpr (DR) {
#pragma unroll
            for (int k = 0; k < 3; ++k) wair[k] = dr[(FD_DR_WIND_N + k) * n + i] + dr[(FD_DR_GUST_N + k) * n + i];
#pragma unroll
            for (int k = 0; k < 5; ++k) dsc[k] = dr[(FD_DR_MASS_S + k) * n + i];
        }
    }
    if constexpr (PREP) {
        if constexpr (EARLY_PARAMS) stage_image_finish(s_params, spw, n_types);
        else stage(s_params, params, n_types * FD_NP_STAGED);
    } else if constexpr (EARLY_PARAMS) stage_params_finish<true>(s_params, spw, n_types);
    else stage_params<false>(s_params, params, n_types);
    if (pid_mode) {
        stage(s_pid_cfg, pid_cfg, 3 * FD_NPC);
        for (int k = threadIdx.x; k < FD_NC; k += blockDim.x) s_consts[k] = S(casc_consts[k]);
    }
    __syncthreads();

    // double-buffered event counters: this launch appends to ev_count[] and clears the OTHER set for the next
    // launch, so the per-step host-side memset disappears from the stream
    if (ev_count_next && blockIdx.x == 0 && threadIdx.x < FD_EV_SHARDS) ev_count_next[threadIdx.x] = 0;

    float o[FD_OBS_DIM];
#pragma unroll
    for (int k = 0; k < FD_OBS_DIM; ++k) o[k] = 0.0f;
    bool done = false, term = false;
    S reward = S(0);

    if (active) {
        const double* blk = s_params + ty * FD_NP_STAGED;
        Params<T> P; P.load(blk);
        if constexpr (DR) scale_params<T>(P, double(dsc[0]), double(dsc[1]), double(dsc[2]), double(dsc[3]), double(dsc[4]));
        Limits<S> Lm; Lm.load(blk);

        // ---- action: from the policy ([n][4] f32, one 16-B load per lane) or the fused rate PID -------------
        float a_in[4];
        S res_bonus = S(0);
        if (!pid_mode) {
            a_in[0] = av.x; a_in[1] = av.y; a_in[2] = av.z; a_in[3] = av.w;
        } else {                                         // learned_controllers/utils/pid_demonstrations.py:47-77
            PidCfg cfg[3]; PidState st[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                cfg[k] = load_pid_cfg(s_pid_cfg, k);
                st[k] = PidState{ pid_state[(k * FD_NPS + 0) * n + i], pid_state[(k * FD_NPS + 1) * n + i], pid_state[(k * FD_NPS + 2) * n + i] };
            }
            const S pid_dt = s_consts[FD_C_PID_DT] > S(0) ? s_consts[FD_C_PID_DT] : ec.dt;
            const Surfaces<S> sf = rate_agent<S>(cfg, st, s_consts, S(e.cmd[0]), S(e.cmd[1]), S(e.cmd[2]), s_consts[FD_C_PID_THROTTLE], x, pid_dt);
            a_in[0] = float(sf.aileron); a_in[1] = float(sf.elevator); a_in[2] = float(sf.rudder); a_in[3] = float(sf.throttle);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                FD_PUT(WT, pid_state[(k * FD_NPS + 0) * n + i], st[k].integral); FD_PUT(WT, pid_state[(k * FD_NPS + 1) * n + i], st[k].err_prev);
                FD_PUT(WT, pid_state[(k * FD_NPS + 2) * n + i], st[k].dfilt);
            }
            if (residual_mode) {                      // float32 arithmetic, as the reference's NumPy float32 arrays
#pragma clang fp contract(off)
                const float rr[4] = { av.x, av.y, av.z, av.w };
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float c = a_in[k] + rr[k] * residual_scale;
                    const float lo = k < 3 ? -1.0f : 0.0f;
                    a_in[k] = c < lo ? lo : (c > 1.0f ? 1.0f : c);
                }
                const float mag = rr[0] * rr[0] + (rr[1] * rr[1] + rr[2] * rr[2]);
                res_bonus = S(0.05) * (S(1) - S(mag) / S(3));   // small-correction bonus (:153-154); fp32 magnitude only
            }
        }
        if constexpr (WT) {                                                       // the wave's rows are one contiguous range
            const int64_t rows = n - lm.wave_first;
            if (actions_out) put16_through(actions_out + lm.wave_first * FD_ACT_DIM, uint32_t(rows < FD_WAVE ? rows : FD_WAVE) * 16u,
                                           uint32_t(lane) * 16u, make_float4(a_in[0], a_in[1], a_in[2], a_in[3]));
        } else if (actions_out) reinterpret_cast<float4*>(actions_out)[i] = make_float4(a_in[0], a_in[1], a_in[2], a_in[3]);
        S a[4];                                                                   // rate_env.py:225
        a[0] = clipv(S(a_in[0]), S(-1), S(1)); a[1] = clipv(S(a_in[1]), S(-1), S(1));
        a[2] = clipv(S(a_in[2]), S(-1), S(1)); a[3] = clipv(S(a_in[3]), S(0), S(1));

        // ---- sim.set_controls + sim.step(dt): n_sub RK4 sub-steps in registers (rate_env.py:228-237) --------
        Controls<T> C;
        C.set(P, a[1], a[0], a[2], a[3]);                                         // action = [ail, elev, rud, thr]
        const S dt_sub = ec.dt / S(ec.n_sub);
#ifdef FD_PHASE_STAMPS
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
        FD_STAMP(1)
        if constexpr (DR) rk4_substeps<S, T, !OCC2, true>(P, Lm, C, x, dt_sub, ec.n_sub, Wind<T>{ T(wair[0]), T(wair[1]), T(wair[2]) });
        else if constexpr (TWO_LOOPS) {
            // The image says that no sub-step of this launch can move an Euler angle by more than 0.125 rad and that no type
            // needs atan2 (Params::euler_increment_bound) -- for states inside the limits every sub-step leaves behind.  A state
            // written from outside need not be: the wave checks the words the bound rests on once, here, and a wave holding such a
            // state (or a non-finite angle) takes the general loop.  Both loops compute the same bits.
            const float r_max = float(Lm.max_rate), p_max = float(Lm.max_pitch);
            const bool outside = !(__builtin_fabsf(float(x[9])) <= r_max) | !(__builtin_fabsf(float(x[10])) <= r_max) |
                                 !(__builtin_fabsf(float(x[11])) <= r_max) | !(__builtin_fabsf(float(x[7])) <= p_max) |
                                 !(__builtin_fabsf(float(x[6])) < __builtin_inff()) | !(__builtin_fabsf(float(x[8])) < __builtin_inff());
            if (small_steps && __ballot(outside) == 0ull) rk4_substeps<S, T, true, false, false>(P, Lm, C, x, dt_sub, ec.n_sub);
            else rk4_substeps<S, T, true>(P, Lm, C, x, dt_sub, ec.n_sub);
        } else rk4_substeps<S, T, !OCC2>(P, Lm, C, x, dt_sub, ec.n_sub);
        FD_STAMP(2)
        if constexpr (sizeof(E) == sizeof(S)) e.time += E(ec.dt);                 // :241-242 (the reference's accumulated sum)
        else e.time = E(S(step + 1) * ec.dt);                                     // fp32 env words: exact product, not an fp32 running sum
        step += 1;

        // ---- _update_command (rate_env.py:342-372) ------------------------------------------------------------
        if (ec.cmd_type == FD_CMD_RAMP) {
            const S t = S(e.time);
            if (t < S(3)) {
                const S alpha = t / S(3);
#pragma unroll
                for (int k = 0; k < 3; ++k) e.cmd[k] = E((S(1) - alpha) * S(0) + alpha * S(e.sched[k]));
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) e.cmd[k] = e.sched[k];
            }
        } else if (ec.cmd_type == FD_CMD_RANDOM_WALK) {
            S delta[3];
            if (rw_delta) {
#pragma unroll
                for (int k = 0; k < 3; ++k) delta[k] = rw_delta[k * n + i];
            } else {                                                              // generators.py:147-164 on device
                Philox ph; uint32_t r[4];
                ph.block(seed, uint32_t(i), uint32_t(episode), uint32_t(step), FD_PHX_RANDOM_WALK, r);
                const float m0 = sqrtf(-2.0f * logf(u01(r[0]))), m1 = sqrtf(-2.0f * logf(u01(r[2])));
                const float n0 = m0 * cosf(6.283185307f * u01(r[1])), n1 = m0 * sinf(6.283185307f * u01(r[1]));
                const float n2 = m1 * cosf(6.283185307f * u01(r[3]));
                const S sd = S(0.1) * M<S>::sqrt(ec.dt) * ec.scale;
                delta[0] = S(n0) * sd * ec.mr0; delta[1] = S(n1) * sd * ec.mr1; delta[2] = S(n2) * sd * ec.mr2;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) e.cmd[k] = E(clipv(S(e.cmd[k]) + delta[k], -ec.max_rate(k), ec.max_rate(k)));
        } else if (ec.cmd_type == FD_CMD_SINE) {
            const S sn = M<S>::sin(S(2.0 * FD_PI) * S(e.sched[3]) * S(e.time));
#pragma unroll
            for (int k = 0; k < 3; ++k) e.cmd[k] = E(S(e.sched[k]) * sn);
        }

        // ---- DR: gust update g <- A g + B n after the physics (first-order Gauss-Markov in NED); the observation, reward and
        // stall test below see the air-mass velocity the next step flies in
        if constexpr (DR) {
            float z[3];
            dr_normals3(seed, uint32_t(i), uint32_t(episode), uint32_t(step), FD_PHX_GUST, z);
            const S ga = dr[FD_DR_GUST_A * n + i], gb = dr[FD_DR_GUST_B * n + i];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const S g = ga * dr[(FD_DR_GUST_N + k) * n + i] + gb * S(z[k]);
                dr[(FD_DR_GUST_N + k) * n + i] = g;
                wair[k] = dr[(FD_DR_WIND_N + k) * n + i] + g;
            }
        }

        // ---- reward, termination (rate_env.py:247-294,437-460) -------------------------------------------------
        // A = arithmetic type of the reward / observation glue: double in the fp64 parity variant, float where the
        // derivatives are evaluated in fp32 anyway (env_reward's header says why the settling timer is exempt)
        using A = typename GlueOf<S, T>::type;
        const A u_ = A(x[3]), v_ = A(x[4]), w_ = A(x[5]), roll_ = A(x[6]), pitch_ = A(x[7]);
        A airspeed = M<A>::sqrt(u_ * u_ + v_ * v_ + w_ * w_);                                // simplified_6dof.py:295-331
        if constexpr (DR) airspeed = air_speed<A, S>(x, wair);                               // DR: air-relative
        const A altitude = -A(x[2]);
        const A err[3] = { A(e.cmd[0]) - A(x[9]), A(e.cmd[1]) - A(x[10]), A(e.cmd[2]) - A(x[11]) };
        const A aa[4] = { A(a[0]), A(a[1]), A(a[2]), A(a[3]) };
        A rew = env_reward<E, A>(e, err, aa, airspeed, altitude, roll_, pitch_, ec.dt, ec.settle_steps);
#pragma unroll
        for (int k = 0; k < 4; ++k) e.prev_action[k] = E(a[k]);                   // :282
        term = (altitude < A(5)) || (M<A>::abs(roll_) > deg2rad<A>(120.0)) || (M<A>::abs(pitch_) > deg2rad<A>(80.0)) ||
               (airspeed < A(8));
        const bool trunc = step >= ec.max_steps;
        if (term && !trunc) rew += A(-100);                                       // :289-292
        reward = S(rew) + res_bonus;
        e.ep_return += E(reward);
        done = term || trunc;
        env_observation<S, A, E>(x, e, airspeed, altitude, o);
        if (reward_f32) reward_f32[i] = float(reward);
        if (reward_full) FD_PUT(WT, reward_full[i], reward);
        terminated[i] = term ? 1 : 0;
        truncated[i] = trunc ? 1 : 0;
    }

    FD_STAMP(3)
    // ---- K4: episode-done compaction -- wave ballot + mbcnt prefix, one atomic per wave ---------------------
    // The returning atomic is ISSUED here and its result consumed only after the auto-reset and the state stores below (the
    // fence in front of the broadcast holds the first use there: left alone, the compiler moves the cross-lane read up into the
    // leader's branch and the wave sits out the whole round trip, behind a full drain of the stores before it).
    const unsigned long long done_mask = __ballot(done);
    const bool compact = done_mask != 0ull && ev_count != nullptr;
    int base = 0, prefix = 0;
    const int shard = int(blockIdx.x) & (FD_EV_SHARDS - 1), cap_s = ev_cap / FD_EV_SHARDS;
    if (compact) {
        const int n_done = __popcll(done_mask);
        prefix = __builtin_amdgcn_mbcnt_hi(uint32_t(done_mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(done_mask), 0u));
        const int leader = __ffsll((long long)done_mask) - 1;
        if (lane == leader) {
            // one lane is already elected: a counter index the compiler takes for per-lane keeps its own wave-level rewrite of
            // uniform atomics off this one (it elects a lane again and reads the result back right behind the atomic)
            int cnt = shard;
            asm volatile("" : "+v"(cnt));
            base = atomicAdd(ev_count + cnt, n_done);
        }
    }
    float o_term[FD_OBS_DIM];                                                     // terminal observation of a finished episode
#pragma unroll
    for (int k = 0; k < FD_OBS_DIM; ++k) o_term[k] = o[k];
    const float ret_term = done ? float(e.ep_return) : 0.0f;
    const int32_t len_term = step;

    // ---- in-kernel auto-reset (vec-env semantics: the returned observation is the post-reset one) -----------
    if (active) {
        if (done && auto_reset) {
            S rec[FD_NR];
            if (pre_drawn) {
#pragma unroll
                for (int k = 0; k < FD_NR; ++k) rec[k] = rec_pre[k];
            } else {
                fetch_reset_record<S>(pool, pool_depth, seed, i, episode, ec, rec);
            }
            env_apply_reset<S, E>(rec, ec.cmd_type, x, e);
            if constexpr (DR) dr_reset<S>(seed, uint32_t(i), uint32_t(episode), drc, EC[FD_EC_DT], dr, n, i, x, wair);
            step = 0;
            episode += 1;
            // first observation of the new episode, in the glue type of this variant (an fp64 square root here is ~400 cycles
            // that three waves in four pay once per launch in the steady state of a random-action fleet)
            using A0 = typename GlueOf<S, T>::type;
            A0 xa[FD_NX];
#pragma unroll
            for (int k = 0; k < FD_NX; ++k) xa[k] = A0(x[k]);
            A0 airspeed, altitude;
            airspeed_altitude<A0>(xa, airspeed, altitude);
            if constexpr (DR) airspeed = air_speed<A0, S>(x, wair);
            env_observation<S, A0, E>(x, e, airspeed, altitude, o);
            if (pid_mode) for (int k = 0; k < 3 * FD_NPS; ++k) FD_PUT(WT, pid_state[k * n + i], 0.0f);   // pid_agent.reset()
        }
#pragma unroll
        for (int k = 0; k < FD_NX; ++k) FD_PUT(WT, xs[k * n + i], x[k]);
        env_store<E>(e, es, n, i, uses_sched);
        eis[FD_EI_STEP * n + i] = step;
        eis[FD_EI_EPISODE * n + i] = episode;
        // The records, still inside the active lanes' block (a finished lane is an active one, the leader among them): on this
        // path the stores above are all younger than the atomic, so the wait in front of its result's first use is a counted
        // one -- at a join with the path of a wave without envs it would be a full drain.
        if (compact) {
            asm volatile("" : "+v"(base) : : "memory");                          // first use: not before this point
            const int leader = __ffsll((long long)done_mask) - 1;
            base = __shfl(base, leader, FD_WAVE);
            const int local = base + prefix;
            if (done && local < cap_s) {
                const int slot = shard * cap_s + local;
                ev_int[slot * FD_EV_NI + FD_EV_ENV] = int32_t(i);
                ev_int[slot * FD_EV_NI + FD_EV_LENGTH] = len_term;
                ev_int[slot * FD_EV_NI + FD_EV_TERMINATED] = term ? 1 : 0;
                ev_flt[slot * FD_EV_NF] = ret_term;
#pragma unroll
                for (int k = 0; k < FD_OBS_DIM; ++k) ev_flt[slot * FD_EV_NF + 1 + k] = o_term[k];
            }
        }
    }
    FD_STAMP(4)
    store_obs_tile<WT>(s_tile[wave], o, lane, obs_out, lm.wave_first, n);
    FD_STAMP(5)
#ifdef FD_PHASE_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    FD_STAMP_REAL(6)
}

// The rate env's prepared launch image (FD_IMG_*): everything the step kernel derives from the parameter table and the env
// constants alone, computed ONCE by the device functions the kernel itself uses (so every word is the one it would compute) --
// the staged parameter blocks with their derived words and the env constants with the sub-step and settle-step counts.  One
// workgroup.  FAST = the fp32-evaluation variants' derived words (Params::derive_lane_from).
static_assert(FD_NIMG == FD_IMG_PARAMS + FD_MAX_TYPES * FD_NP_STAGED && FD_ECD_INTS + 2 <= FD_ECD_SMALL_STEPS &&
              FD_ECD_SMALL_STEPS < FD_IMG_PARAMS, "fdyn_layout.h: image sections");
template <bool FAST>
__global__ void __launch_bounds__(FD_BLOCK)
rate_env_image_kernel(const double* __restrict__ params, int n_types, const double* __restrict__ EC, double* __restrict__ image)
{
    double* blocks = image + FD_IMG_PARAMS;
    for (int i = threadIdx.x; i < FD_MAX_TYPES * FD_NP_STAGED; i += blockDim.x) {
        const int t = i / FD_NP_STAGED, k = i - t * FD_NP_STAGED;
        blocks[i] = (t < n_types && k < FD_NP_USED) ? params[t * FD_NP + k] : 0.0;
    }
    for (int k = threadIdx.x; k < FD_IMG_PARAMS; k += blockDim.x) if ((k < FD_ECD_INTS || k >= FD_ECD_INTS + 2) && k != FD_ECD_SMALL_STEPS) image[FD_IMG_EC + k] = k < FD_NEC ? EC[k] : 0.0;
    __syncthreads();                                               // the derived words below land on the zeros above
    constexpr int NDL = Params<double>::FD_ND_LANES;
    if (int(threadIdx.x) < n_types * NDL) {
        const int t = threadIdx.x / NDL;
        Params<double>::derive_lane<FAST>(threadIdx.x - t * NDL, params + t * FD_NP, blocks + t * FD_NP_STAGED);
    }
    if (threadIdx.x == FD_BLOCK - 1) {
        EnvConsts<double> ec;
        load_env_consts<double>(EC, ec);
        int32_t* ic = reinterpret_cast<int32_t*>(image + FD_IMG_EC + FD_ECD_INTS);
        ic[0] = ec.max_steps; ic[1] = ec.cmd_type; ic[2] = ec.n_sub; ic[3] = ec.settle_steps;
        // FD_ECD_SMALL_STEPS: the step kernel may run the sub-step loop without dynamics_fast's rare block (the alpha test is
        // derive lane 5's, on the same fp32 sin / cos)
        bool small = FAST;
        if constexpr (FAST) {
            const double dt_sub = ec.dt / double(ec.n_sub);
            for (int t = 0; t < n_types; ++t) {
                const double* src = params + t * FD_NP;
                const double a = src[FD_P_MAX_ALPHA_RAD];
                float snf, csf;
                fast::sincos(float(a), snf, csf);
                const bool poly_ok = a > 0.0 && a < 1.5 && double(snf) / double(csf) <= double(FD_ATAN_WIDE_LIMIT);
                small = small && poly_ok && Params<double>::small_steps_ok(src, dt_sub);
            }
        }
        image[FD_IMG_EC + FD_ECD_SMALL_STEPS] = small ? 1.0 : 0.0;
    }
}

// =========================================================================================================
// C-ABI (include/fdyn.h)
// =========================================================================================================
static int g_simds = 0;
static int simd_count()
{
    if (!g_simds) {
        int dev = 0; hipDeviceProp_t p;
        g_simds = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) ? p.multiProcessorCount * 4 : 1024;
    }
    return g_simds;
}

// The rate env's reset and step, plain and with domain randomisation (DRA = S* dr [FD_NDR][n], const double* dr_consts [FD_NDC]):
// the parameters they share are spelled once, the entry points below forward to one host function each.
#define FD_ENV_RESET_PARAMS(S, E)                                                                            \
    S* x, E* e, int32_t* ei, float* pid_state, const uint8_t* mask, const double* env_consts, const double* pool, \
    int pool_depth, uint64_t seed, float* obs_out, int64_t n
#define FD_ENV_RESET_ARGS x, e, ei, pid_state, mask, env_consts, pool, pool_depth, seed, obs_out, n
#define FD_ENV_STEP_PARAMS(S, E)                                                                             \
    S* x, E* e, int32_t* ei, const uint8_t* type, const double* params, int n_types, const double* env_consts, \
    const float* actions, float* pid_state, const float* pid_cfg, const double* casc_consts, float* actions_out, \
    const S* rw_delta, const double* pool, int pool_depth, uint64_t seed, int auto_reset, float residual_scale, \
    float* obs_out, float* reward_f32, S* reward_full, uint8_t* terminated, uint8_t* truncated, int32_t* ev_count, \
    int32_t* ev_count_next, int32_t* ev_int, float* ev_flt, int ev_cap, int64_t n
#define FD_ENV_STEP_ARGS                                                                                     \
    x, e, ei, type, params, n_types, env_consts, actions, pid_state, pid_cfg, casc_consts, actions_out, rw_delta, pool, \
    pool_depth, seed, auto_reset, residual_scale, obs_out, reward_f32, reward_full, terminated, truncated, ev_count, \
    ev_count_next, ev_int, ev_flt, ev_cap, n

template <typename S, typename E, typename... DRA>
static int env_reset(FD_ENV_RESET_PARAMS(S, E), void* stream, DRA... dra)
{
    if ((... || !dra)) return FDYN_ERR_NULL;
    FD_CHECK_FLEET(n, 1, FD_BLOCK)
    if (pool && pool_depth < 1) return FDYN_ERR_BAD_SIZE;
    return launch<FD_BLOCK>(rate_env_reset_kernel<S, E, DRA...>, n, stream, FD_ENV_RESET_ARGS, dra...);
}

template <typename S, typename E, typename T, bool PREP, typename... DRA>
static int env_step(FD_ENV_STEP_PARAMS(S, E), void* stream, DRA... dra)
{
    if ((... || !dra)) return FDYN_ERR_NULL;
    FD_CHECK_FLEET(n, n_types, FD_BLOCK)
    if (pool && pool_depth < 1) return FDYN_ERR_BAD_SIZE;
    if ((!actions || residual_scale > 0.0f) && !(pid_state && pid_cfg && casc_consts)) return FDYN_ERR_NULL;
    if (!obs_out || !terminated || !truncated || !env_consts) return FDYN_ERR_NULL;
    if (ev_count && (!ev_int || !ev_flt)) return FDYN_ERR_NULL;
    // records go to FD_EV_SHARDS equal segments: a capacity that is not a positive multiple would give segments of zero (or
    // fewer than stated) records and drop episode ends silently
    if (ev_count && (ev_cap < FD_EV_SHARDS || ev_cap % FD_EV_SHARDS != 0)) return FDYN_ERR_BAD_SIZE;
    // fp32 arithmetic and more than one wave per SIMD: the register-capped build, two workgroups per CU (the f64 build is
    // never register-capped: its flag is false on both sides, no fp64 OCC2 instantiation)
    constexpr bool FP32 = sizeof(T) == 4;
    const bool occ2 = FP32 && n > int64_t(simd_count()) * FD_WAVE;
    return launch<FD_BLOCK>(occ2 ? rate_env_step_kernel<S, T, FP32, PREP, DRA...> : rate_env_step_kernel<S, T, false, PREP, DRA...>,
                            n, stream, FD_ENV_STEP_ARGS, dra...);
}

extern "C" {

int fdyn_abi_version(void) { return FDYN_ABI_VERSION; }

int fdyn_num_substeps(double dt, double dt_physics)
{   // simulation/simulation_backend.py:95  max(1, int(dt / dt_physics))
    const double r = dt / dt_physics;
    const long n = long(r);
    return n < 1 ? 1 : int(n);
}

int64_t fdyn_event_capacity(int64_t n)
{   // every shard must hold all the envs of the workgroups that map to it
    const int64_t blocks = (n + FD_BLOCK - 1) / FD_BLOCK;
    return FD_EV_SHARDS * ((blocks + FD_EV_SHARDS - 1) / FD_EV_SHARDS) * FD_BLOCK;
}

int fdyn_device_info(int* cu_count, int* wave_size, char* arch, int arch_len)
{
    hipDeviceProp_t p;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return int(e);
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return int(e);
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (wave_size) *wave_size = p.warpSize;
    if (arch && arch_len > 0) { strncpy(arch, p.gcnArchName, arch_len - 1); arch[arch_len - 1] = 0; }
    return FDYN_OK;
}

#define FD_DEFINE_SIXDOF(NAME, S, T)                                                                         \
    int NAME(S* x, const S* u, const uint8_t* type, const double* params, int n_types, int64_t n, double dt, \
             int n_sub, S* derived_out, void* stream)                                                        \
    {                                                                                                        \
        FD_CHECK_FLEET(n, n_types, FD_BLOCK)                                                                 \
        if (n_sub < 1) return FDYN_ERR_BAD_SIZE;                                                             \
        const double dt_sub = dt / n_sub;                                                                    \
        if (bad_dt(dt_sub)) return FDYN_ERR_BAD_DT;                                                          \
        return launch<FD_BLOCK>(sixdof_step_kernel<S, T>, n, stream, x, u, type, params, n_types, n, S(dt_sub), n_sub,   \
                                derived_out);                                                                \
    }
FD_DEFINE_SIXDOF(fdyn_sixdof_step_f64, double, double)
FD_DEFINE_SIXDOF(fdyn_sixdof_step_mixed, double, float)
FD_DEFINE_SIXDOF(fdyn_sixdof_step_f32, float, float)

int fdyn_derived_f64(const double* x, int64_t n, double* out, void* stream)
{
    FD_CHECK_FLEET(n, 1, FD_BLOCK)
    return launch<FD_BLOCK>(derived_kernel<double>, n, stream, x, n, out);
}
int fdyn_derived_f32(const float* x, int64_t n, float* out, void* stream)
{
    FD_CHECK_FLEET(n, 1, FD_BLOCK)
    return launch<FD_BLOCK>(derived_kernel<float>, n, stream, x, n, out);
}

int fdyn_pid_compute_batch(const float* cfg, int cfg_per_lane, float* state, const float* setpoint,
                           const float* measurement, float dt, float* out, int64_t n, void* stream)
{
    FD_CHECK_FLEET(n, 1, FD_BLOCK)
    return launch<FD_BLOCK>(pid_batch_kernel, n, stream, cfg, cfg_per_lane, state, setpoint, measurement, dt, out, n);
}

#define FD_DEFINE_CASCADE(NAME, S, T)                                                                        \
    int NAME(S* x, float* pid_state, int32_t* wp_idx, const uint8_t* type, const double* params, int n_types, \
             const float* pid_cfg, const double* consts, const double* wps, int n_wp, int64_t n, double dt,  \
             int n_steps, S* surf_out, int32_t* reached_total, void* stream)                                 \
    {                                                                                                        \
        FD_CHECK_FLEET(n, n_types, FD_BLOCK)                                                                 \
        if (n_wp < 1 || n_wp > FD_MAX_WAYPOINTS || n_steps < 0) return FDYN_ERR_BAD_SIZE;                    \
        if (bad_dt(dt)) return FDYN_ERR_BAD_DT;                                                              \
        return launch<FD_BLOCK>(cascade_step_kernel<S, T>, n, stream, x, pid_state, wp_idx, type, params, n_types, pid_cfg, \
                                consts, wps, n_wp, n, S(dt), n_steps, surf_out, reached_total);              \
    }
#define FD_DEFINE_AGENT(NAME, S, T)                                                                          \
    int NAME(int level, S* x, float* pid_state, const uint8_t* type, const double* params, int n_types,      \
             const float* pid_cfg, int cfg_per_lane, const double* consts, const S* cmd, int64_t n, double dt, \
             int n_steps, S* surf_out, void* stream)                                                         \
    {                                                                                                        \
        FD_CHECK_FLEET(n, n_types, FD_BLOCK)                                                                 \
        if (level < FD_LEVEL_WAYPOINT || level > FD_LEVEL_RATE || n_steps < 0) return FDYN_ERR_BAD_SIZE;     \
        if (n > 0 && (!x || !pid_state || !pid_cfg || !consts || !cmd)) return FDYN_ERR_NULL;                \
        if (bad_dt(dt)) return FDYN_ERR_BAD_DT;                                                              \
        return launch<FD_BLOCK>(agent_step_kernel<S, T>, n, stream, level, x, pid_state, type, params, n_types, pid_cfg, \
                                consts, cmd, n, S(dt), n_steps, surf_out, cfg_per_lane);                     \
    }
FD_DEFINE_AGENT(fdyn_agent_step_f64, double, double)
FD_DEFINE_AGENT(fdyn_agent_step_mixed, double, float)
FD_DEFINE_AGENT(fdyn_agent_step_f32, float, float)

#define FD_DEFINE_HYBRID(NAME, S, T)                                                                         \
    int NAME(int level, S* x, float* pid_state, int32_t* wp_idx, const uint8_t* type, const double* params, int n_types, \
             const float* pid_cfg, const double* consts, const S* cmd, const double* wps, int n_wp, const float* actions, \
             const uint8_t* learned, int throttle_src, float* prev_action, float* obs_out, float* rate_cmd_out,  \
             S* surf_out, int32_t* reached_total, int64_t n, double dt, void* stream)                         \
    {                                                                                                        \
        FD_CHECK_FLEET(n, n_types, FD_BLOCK)                                                                 \
        if (level != FD_LEVEL_WAYPOINT && level != FD_LEVEL_HSA && level != FD_LEVEL_ATTITUDE) return FDYN_ERR_BAD_SIZE; \
        if (throttle_src != FD_HYBRID_THROTTLE_POLICY && throttle_src != FD_HYBRID_THROTTLE_OUTER) return FDYN_ERR_BAD_SIZE; \
        if (wps && (level != FD_LEVEL_WAYPOINT || n_wp < 1 || n_wp > FD_MAX_WAYPOINTS || cmd)) return FDYN_ERR_BAD_SIZE; \
        if (!wps && n_wp != 0) return FDYN_ERR_BAD_SIZE;                                                     \
        if (!x || !pid_state || !params || !pid_cfg || !consts || !prev_action || !obs_out || !surf_out)     \
            return FDYN_ERR_NULL;                                                                            \
        if (wps ? !wp_idx : !cmd) return FDYN_ERR_NULL;                                                      \
        if (bad_dt(dt)) return FDYN_ERR_BAD_DT;                                                              \
        return launch<FD_BLOCK>(hybrid_step_kernel<S, T>, n, stream, level, x, pid_state, wp_idx, type, params, n_types, \
                                pid_cfg, consts, cmd, wps, n_wp, actions, learned, throttle_src, prev_action, obs_out, \
                                rate_cmd_out, surf_out, reached_total, n, S(dt));                            \
    }
FD_DEFINE_HYBRID(fdyn_hybrid_step_f64, double, double)
FD_DEFINE_HYBRID(fdyn_hybrid_step_mixed, double, float)
FD_DEFINE_HYBRID(fdyn_hybrid_step_f32, float, float)

FD_DEFINE_CASCADE(fdyn_cascade_step_f64, double, double)
FD_DEFINE_CASCADE(fdyn_cascade_step_mixed, double, float)
FD_DEFINE_CASCADE(fdyn_cascade_step_f32, float, float)

#define FD_DEFINE_ENV(SUFFIX, S, E, T)                                                                       \
    int fdyn_rate_env_reset_##SUFFIX(FD_ENV_RESET_PARAMS(S, E), void* stream)                                \
    { return env_reset<S, E>(FD_ENV_RESET_ARGS, stream); }                                                   \
    int fdyn_rate_env_step_##SUFFIX(FD_ENV_STEP_PARAMS(S, E), void* stream)                                  \
    { return env_step<S, E, T, false>(FD_ENV_STEP_ARGS, stream); }
FD_DEFINE_ENV(f64, double, double, double)
FD_DEFINE_ENV(mixed, double, float, float)
FD_DEFINE_ENV(f32, float, float, float)

#define FD_DEFINE_ENV_DR(SUFFIX, S, E, T)                                                                    \
    int fdyn_rate_env_reset_dr_##SUFFIX(FD_ENV_RESET_PARAMS(S, E), S* dr, const double* dr_consts, void* stream) \
    { return env_reset<S, E>(FD_ENV_RESET_ARGS, stream, dr, dr_consts); }                                    \
    int fdyn_rate_env_step_dr_##SUFFIX(FD_ENV_STEP_PARAMS(S, E), S* dr, const double* dr_consts, void* stream) \
    { return env_step<S, E, T, false>(FD_ENV_STEP_ARGS, stream, dr, dr_consts); }
FD_DEFINE_ENV_DR(f64, double, double, double)
FD_DEFINE_ENV_DR(mixed, double, float, float)
FD_DEFINE_ENV_DR(f32, float, float, float)

// The prepared launch image of the rate env and the step entry points that take it: `params` and `env_consts` of the _img entry
// points are not read, the kernel gets the image's two sections in their place.
int fdyn_rate_env_image(const double* params, int n_types, const double* env_consts, int fp32_eval, double* image, void* stream)
{
    if (n_types < 1 || n_types > FD_MAX_TYPES) return FDYN_ERR_BAD_TYPES;
    if (!params || !env_consts || !image) return FDYN_ERR_NULL;
    return launch<FD_BLOCK>(fp32_eval ? rate_env_image_kernel<true> : rate_env_image_kernel<false>, FD_BLOCK, stream, params,
                            n_types, env_consts, image);
}
#define FD_DEFINE_ENV_IMG(SUFFIX, S, E, T)                                                                   \
    int fdyn_rate_env_step_img_##SUFFIX(FD_ENV_STEP_PARAMS(S, E), const double* image, void* stream)         \
    {                                                                                                        \
        if (!image) return FDYN_ERR_NULL;                                                                    \
        params = image + FD_IMG_PARAMS; env_consts = image + FD_IMG_EC;                                      \
        return env_step<S, E, T, true>(FD_ENV_STEP_ARGS, stream);                                            \
    }                                                                                                        \
    int fdyn_rate_env_step_dr_img_##SUFFIX(FD_ENV_STEP_PARAMS(S, E), S* dr, const double* dr_consts, const double* image, \
                                           void* stream)                                                     \
    {                                                                                                        \
        if (!image) return FDYN_ERR_NULL;                                                                    \
        params = image + FD_IMG_PARAMS; env_consts = image + FD_IMG_EC;                                      \
        return env_step<S, E, T, true>(FD_ENV_STEP_ARGS, stream, dr, dr_consts);                             \
    }
FD_DEFINE_ENV_IMG(f64, double, double, double)
FD_DEFINE_ENV_IMG(mixed, double, float, float)
FD_DEFINE_ENV_IMG(f32, float, float, float)

}  // extern "C"
