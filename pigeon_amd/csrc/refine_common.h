// refine_common.h -- the two device helpers of the refiner's selection, one definition each: refine_select_kernel (refine.hip) and the
// grid sweep (refine_sweep.hip) both include this file, and both files are compiled with the same flags (the compiler's default
// contraction), because a grid point of pg_refine_sweep must be pg_refine_forward's choice bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

// torch.argmax semantics over n <= 64 values: first maximum; a NaN is the maximum (first NaN wins).
__device__ __forceinline__ int argmax_torch(const float* v, int n) {
    int bi = 0; float bv = v[0];
    for (int i = 1; i < n; ++i) {
        const float x = v[i];
        if (bv != bv) break;                                // already NaN -> stays
        if (x != x || x > bv) { bv = x; bi = i; }
    }
    return bi;
}

// The veto distance with the reference's dtype promotion.  models/proto_refiner.py:198-202 calls
// haversine(initial_LLH, refined_LLH) (preprocessing/geo_utils.py:40-55) with x = the float64 initial prediction and
// y = torch.tensor(top_preds[...]) = a FLOAT32 tensor: torch.deg2rad(y) and torch.cos(y_rad[:,1]) are evaluated in fp32
// (deg2rad multiplies by pi/180 rounded to the tensor dtype), `y_rad - x_rad` and everything after promote to float64.
// cos of the fp32 latitude is taken as the correctly rounded fp32 value (double cos, rounded once): torch's CPU kernel
// (Sleef, <= 1 ulp) agrees with it except for rare last-bit cases, which no device libm could reproduce anyway.
__device__ __forceinline__ double haversine_km(double lng1, double lat1, float lng2, float lat2) {
    const double d2r = 0.017453292519943295769236907684886127134428718885417;   // M_PI / 180
    const double x0 = lng1 * d2r, x1 = lat1 * d2r;
    const float y0 = lng2 * (float)d2r, y1 = lat2 * (float)d2r;                  // fp32 deg2rad
    const double dl = (double)y0 - x0, dp = (double)y1 - x1;
    const double sp = sin(dp / 2), sl = sin(dl / 2);
    const float cy = (float)cos((double)y1);                                      // fp32 cos(lat of the refined point)
    const double a = sp * sp + cos(x1) * (double)cy * (sl * sl);
    const double c = 2 * asin(sqrt(a));
    return (6378137.0 * c) / 1000;
}
