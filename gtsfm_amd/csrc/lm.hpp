// Host control flow of the Levenberg-Marquardt solvers whose linear solve is a preconditioned conjugate gradient
// (gba.hip, transavg.hip): GTSAM's accept test and lambda schedule, the outer stop test and the PCG iteration loop.
// Which kernels a trial launches and when it reads the device stay with each solver; only the decisions are here.
// ba2.hip runs the same schedule on the device and takes the constants. Sets no fp-contract pragma: include it after
// the includer's own (see se3.hpp).
#pragma once
#include <math.h>

#include "common.hpp"

namespace {

constexpr double kMinFidelity = 1e-3;
constexpr double kLambdaUpper = 1e5;
constexpr double kDblEps = 2.220446049250313e-16;
constexpr int kInnerMax = 64;  // trials per outer iteration

struct LmTrial {
    bool success = false, stop = false;
    double newErr = INFINITY;
};

// The verdict on a solved trial step: err is the current error, oldLin / newLin the linearised cost before and after
// the step, stepErr the nonlinear error at the step. A step that raises the linearised cost is rejected unseen.
inline LmTrial lm_judge(double err, double oldLin, double newLin, double stepErr) {
    LmTrial t;
    const double linChange = oldLin - newLin;
    if (linChange >= 0) {
        t.newErr = stepErr;
        const double costChange = err - t.newErr;
        if (linChange > kDblEps * oldLin) t.success = costChange / linChange > kMinFidelity;
        else t.success = true;
        if (fabs(costChange) < 1e-5 * err) t.stop = true;
    }
    return t;
}

// Closes a trial: an accepted step divides lambda by 10, a rejected one multiplies it by 10. True when the trial loop
// ends: the step was accepted, the stop test fired, or lambda reached its upper bound.
inline bool lm_trials_done(const LmTrial& t, double& lambda) {
    if (t.success) {
        lambda /= 10.0;
        return true;
    }
    if (t.stop) return true;
    lambda *= 10.0;
    return lambda >= kLambdaUpper;
}

// The outer stop test after the trials of one linearisation: cur is the error before them, err the error now.
inline bool lm_done(double cur, double err, long long iters, int max_iters) {
    const double dec = cur - err;
    return iters >= max_iters || dec / cur <= 1e-5 || dec <= 1e-5 || !isfinite(cur);
}

// PCG until ||r|| <= rel_tol ||b|| (rr = |r|^2, bb = |b|^2) or max_iter iterations, which counts one cap hit; a
// non-finite residual ends the solve, the step then fails the accept test. step(rr) launches one iteration and reads
// the new |r|^2 into rr; its return code ends the solve when it is not GTSFM_OK. iters grows by the iterations made.
template <class Step>
int pcg_iterate(double bb, double rr, double rel_tol, int max_iter, long long& iters, long long& cap_hits, Step step) {
    int k = 0;
    while (isfinite(rr) && !(sqrt(rr) <= rel_tol * sqrt(bb))) {
        if (k >= max_iter) {
            ++cap_hits;
            break;
        }
        const int rc = step(rr);
        if (rc != GTSFM_OK) return rc;
        ++k;
    }
    iters += k;
    return GTSFM_OK;
}

}  // namespace
