// The curvature of a Poincare-ball entry point (pmath.hip, pmath_grad.hip).  An operation is exported twice: the float
// form takes c by value, the _c form reads ONE float c_dev on the device and, in a backward pass, gives it a gradient (gc_ws: the rows'
// float64 shares, gc [1]: their sum, WRITTEN by pmath_gc_finish_kernel).  Both forward to one host function, which takes the curvature
// as a Curv and the called entry's name as `who`; where the two forms differ, that function branches on cv.dev.
#pragma once
#include "api_util.hpp"

struct Curv {
    float c;              // the float form's value; 0 in the device form (the kernels then read *c_dev)
    const float* c_dev;   // the device form's curvature; NULL in the float form
    double* gc_ws;        // backward, device form: workspace of dL/dc
    float* gc;            // backward, device form: dL/dc
    bool dev;             // the _c entry was called (c_dev itself may still be NULL: that is the form's first refusal)
};
static inline Curv curv_float(float c) { return Curv{c, nullptr, nullptr, nullptr, false}; }
static inline Curv curv_dev(const float* c_dev, double* gc_ws = nullptr, float* gc = nullptr) { return Curv{0.f, c_dev, gc_ws, gc, true}; }

// refusals of a function that has `who` and `cv` in scope
#define PM_REQUIRE(cond, why)                      \
    do {                                           \
        if (!(cond)) return stt_refuse(who, why);  \
    } while (0)
#define PM_REQUIRE_CURV() PM_REQUIRE(!cv.dev || cv.c_dev, "c_dev is NULL (the curvature is read from the device)")
