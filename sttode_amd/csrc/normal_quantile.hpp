// The standard normal quantile in float64: Wichura's algorithm AS241, routine PPND16 (Appl. Statist. 37, 1988), relative error about 1e-16.
// Host and device: the latent-set generator (latents.hip) evaluates it per drawn value and rounds the result to float32 once.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

// Phi^-1(0.5 + q) for q = p - 0.5 handed over as such: PPND16 works on q anyway, and a caller that has q to full precision (a value near the
// mode, where 0.5 + q would round most of q away) keeps it.  |q| <= 0.5 - 2^-33 -- what (x + 0.5) 2^-32 of a 32-bit x gives, truncated or
// not.  There r = sqrt(-log(0.5 - |q|)) <= 4.79, so PPND16's third rational (r > 5, p below 1.4e-11) is never reached and is left out.
__host__ __device__ inline double stt_ppnd16(double q) {
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2509.0809287301226727 * r + 33430.575583588128105) * r + 67265.770927008700853) * r + 45921.953931549871457) * r +
                               13731.693765509461125) * r + 1971.5909503065514427) * r + 133.14166789178437745) * r + 3.387132872796366608);
        const double den = (((((((5226.495278852545925 * r + 28729.085735721942674) * r + 39307.89580009271061) * r + 21213.794301586595867) * r +
                               5394.1960214247511077) * r + 687.1870074920579083) * r + 42.313330701600911252) * r + 1.0);
        return q * num / den;
    }
    const double r = sqrt(-log(0.5 - fabs(q))) - 1.6;             // 0.5 - |q| = min(p, 1 - p), exact for |q| >= 0.25
    const double num = (((((((7.7454501427834140764e-4 * r + 0.0227238449892691845833) * r + 0.24178072517745061177) * r + 1.27045825245236838258) * r +
                           3.64784832476320460504) * r + 5.7694972214606914055) * r + 4.6303378461565452959) * r + 1.42343711074968357734);
    const double den = (((((((1.05075007164441684324e-9 * r + 5.475938084995344946e-4) * r + 0.0151986665636164571966) * r + 0.14810397642748007459) * r +
                           0.68976733498510000455) * r + 1.6763848301838038494) * r + 2.05319162663775882187) * r + 1.0);
    const double v = num / den;
    return q < 0.0 ? -v : v;
}
