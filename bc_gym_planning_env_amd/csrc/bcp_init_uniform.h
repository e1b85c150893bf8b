// bcp_init_uniform.h -- the declared uniform initial state (bcp_declare_uniform_initial_state; include/bcplan.h): the block of
// the step's parameters that holds ONE initial state for every env (InitUniform, a member of StepStatic in bcp_step.h), the
// bit-for-bit comparison of the eleven initial-state arrays against their entry 0, and the packing of that entry.  Plain C++
// with no HIP in it: the declaration (bcp_seams_host.h) calls init_uniform_pack on the host copies of the caller's arrays,
// tests/c_abi/init_uniform_main.cpp calls the same function under the sanitizers, and there is no other copy of it.
#pragma once

#include <cstdint>
#include <cstring>

namespace bcp {

// One initial state, as the finishing pass of the step kernel takes it (InitAhead, bcp_step.h).  80 bytes, five 16-byte pieces
// of the parameter block: step_local_kernel stages it in LDS with the rest of *S.  `on` is informative (the kernels look at the
// launch flag kStepInitUniform, never at this word).
struct InitUniform {
    double x, y, th, v, w, steer, wheel, min_dist;
    int32_t target, iter, collided, on;
};
static_assert(sizeof(InitUniform) == 80, "five 16-byte pieces of the parameter block");

// the eleven arrays in the order of bcp_state (x .. robot_collided)
enum InitField {
    kInitX = 0, kInitY, kInitAngle, kInitV, kInitW, kInitSteer, kInitWheel, kInitMinDist, kInitTarget, kInitIter, kInitCollided,
    kInitFields
};

inline const char* init_field_name(int field)
{
    static const char* const names[kInitFields] = {"x", "y", "angle", "v", "w", "steering_motor_command", "wheel_angle",
                                                   "min_spat_dist_so_far", "target_idx", "current_iter", "robot_collided"};
    return field >= 0 && field < kInitFields ? names[field] : "?";
}

// host copies of the arrays, n entries each (steer and wheel may be null when the model is not the tricycle's)
struct InitHostArrays {
    const double* f64[8];      // x, y, angle, v, w, steer, wheel, min_dist
    const int32_t* target;
    const int32_t* iter;
    const uint8_t* collided;
};

// the first entry that is not entry 0, and the first of its fields that differs; env < 0: every entry agrees
struct InitDifference {
    int64_t env;
    int field;
};

// a double as its 64-bit word: NaNs compare by payload, -0.0 is not 0.0
inline uint64_t init_word(double v)
{
    uint64_t w;
    std::memcpy(&w, &v, sizeof(w));
    return w;
}

// Compares entries 1 .. n - 1 with entry 0, bit for bit, and packs entry 0 into *out (always, n >= 1: the caller keeps it only
// when the result says "uniform").  tri = false (the diff-drive model): steer and wheel are neither read nor compared, the
// snapshot holds 0.0 for both and the kernels do not restore them.
inline InitDifference init_uniform_pack(const InitHostArrays& a, int64_t n, bool tri, InitUniform* out)
{
    InitDifference none = {-1, -1};
    if (n < 1) return none;
    std::memset(out, 0, sizeof(*out));   // (the padding-free struct, the two tricycle values of a diff-drive robot)
    double* const packed[8] = {&out->x, &out->y, &out->th, &out->v, &out->w, &out->steer, &out->wheel, &out->min_dist};
    for (int f = 0; f < 8; ++f) {
        const bool tricycle_only = f == kInitSteer || f == kInitWheel;
        if (tricycle_only && !tri) continue;
        *packed[f] = a.f64[f][0];
    }
    out->target = a.target[0];
    out->iter = a.iter[0];
    out->collided = (int32_t)a.collided[0];
    out->on = 1;
    for (int64_t i = 1; i < n; ++i) {
        for (int f = 0; f < 8; ++f) {
            const bool tricycle_only = f == kInitSteer || f == kInitWheel;
            if (tricycle_only && !tri) continue;
            if (init_word(a.f64[f][i]) != init_word(a.f64[f][0])) return InitDifference{i, f};
        }
        if (a.target[i] != a.target[0]) return InitDifference{i, kInitTarget};
        if (a.iter[i] != a.iter[0]) return InitDifference{i, kInitIter};
        if (a.collided[i] != a.collided[0]) return InitDifference{i, kInitCollided};
    }
    return none;
}

}  // namespace bcp
