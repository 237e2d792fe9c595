// haversine.h -- the ONE device definition of the great-circle distance (reference preprocessing/geo_utils.py:58-74) that
// pg_haversine_matrix (geo_proto.hip) and pg_guess_spread (spread.hip) evaluate.  Both files are compiled with the same flags (the
// compiler's default contraction), and a radius of pg_guess_spread is, bit for bit, an element of pg_haversine_matrix plus the
// cell's extent: tests/test_gpu_spread.py holds the two against each other at zero tolerance, tests/test_gpu_geo.py holds the
// matrix to its own statement (csrc/optics.hip restates the fp64 arm once more, with the same two fused operations written out).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

// the score of a distance d km is PG_SCORE_MAX * exp(-d / PG_SCORE_DECAY_KM).  Constants only: spread.hip and guess_best.hip associate
// the product differently, and each expression's bits are part of its contract.
#define PG_SCORE_MAX 5000.0
#define PG_SCORE_DECAY_KM 1492.7                     // pigeon_amd/config.py DECAY_CONSTANT

// torch.deg2rad multiplies by the double constant pi/180 rounded to the tensor's dtype
#define DEG2RAD_D 0.017453292519943295769236907684886127134428718885417
template <typename X> struct Deg;
template <> struct Deg<double> {
    static __device__ __forceinline__ double rad(double v) { return v * DEG2RAD_D; }
    static __device__ __forceinline__ double cosv(double r) { return cos(r); }
};
template <> struct Deg<float> {
    static __device__ __forceinline__ float rad(float v) { return v * (float)DEG2RAD_D; }
    static __device__ __forceinline__ float cosv(float r) { return (float)cos((double)r); }   // correctly rounded fp32 cos
};

// x = [lng, lat] degrees in fp32 (deg2rad and cos(lat) evaluated in fp32, then promoted: torch's dtype rules), y fp64 -> km.  The fp32
// arm is what pg_haversine_matrix alone runs; its contraction is the compiler's, as it always was.
template <typename X>
__device__ __forceinline__ double pg_haversine_km(X xlng_deg, X xlat_deg, double ylng_deg, double ylat_deg) {
    const X xlng = Deg<X>::rad(xlng_deg), xlat = Deg<X>::rad(xlat_deg);
    const double ylng = ylng_deg * DEG2RAD_D, ylat = ylat_deg * DEG2RAD_D;
    const double dlng = (double)xlng - ylng, dlat = (double)xlat - ylat;
    const double p = (double)Deg<X>::cosv(xlat) * cos(ylat);
    const double s1 = sin(dlat / 2), s0 = sin(dlng / 2);
    const double a = s1 * s1 + p * (s0 * s0);
    const double c = 2 * asin(sqrt(a));
    return (6378137.0 * c) / 1000;
}

// The fp64 arm, which both files run.  Left to the compiler, which products are fused into the additions that follow them depends on
// the CALL SITE (a point that is constant across a loop has its multiplication hoisted, and the other operand's is fused instead), so
// the two operations the matrix kernel's code object has always fused -- the longitude difference, on x's side, and the sum under
// the root -- are written as fma() and nothing else may be contracted: the same bits wherever this is inlined.
template <>
__device__ __forceinline__ double pg_haversine_km<double>(double xlng_deg, double xlat_deg, double ylng_deg, double ylat_deg) {
#pragma clang fp contract(off)
    const double xlat = xlat_deg * DEG2RAD_D;
    const double ylng = ylng_deg * DEG2RAD_D, ylat = ylat_deg * DEG2RAD_D;
    const double dlng = fma(xlng_deg, DEG2RAD_D, -ylng), dlat = xlat - ylat;
    const double p = cos(xlat) * cos(ylat);
    const double s1 = sin(dlat / 2), s0 = sin(dlng / 2);
    const double a = fma(s1, s1, p * (s0 * s0));
    const double c = 2 * asin(sqrt(a));
    return (6378137.0 * c) / 1000;
}
