/* Linear interpolation under GSL's names, our own text: what the AWGN half of the vendored
 * CapacityEvaluator.cpp calls from its constructors and destructor. It runs at start-up of
 * every polar_ref process, for the capacity tables of the library's built-in "G" and "A5"
 * kernels (TruncatedArikanKernel.cpp's global objects). Nothing it computes is recorded in a
 * fixture: the product has no AWGN interpolator, and a fixture would pin this file to itself.
 * Outside [xa[0], xa[size-1]] the value is that of the nearest end (GSL raises a domain error
 * there; the library clamps the argument to [0, 1] before it calls). */
#pragma once
#include <cstddef>

struct gsl_interp_type {
    int min_size;
};
static const gsl_interp_type bchk_shim_interp_linear = {2};
static const gsl_interp_type *const gsl_interp_linear = &bchk_shim_interp_linear;

struct gsl_interp {
    size_t size;
};
struct gsl_interp_accel {
    size_t cache;  /* the last interval found */
};

inline gsl_interp *gsl_interp_alloc(const gsl_interp_type *, size_t size) { return new gsl_interp{size}; }
inline int gsl_interp_init(gsl_interp *it, const double *, const double *, size_t size) {
    it->size = size;
    return 0;
}
inline void gsl_interp_free(gsl_interp *it) { delete it; }
inline gsl_interp_accel *gsl_interp_accel_alloc() { return new gsl_interp_accel{0}; }
inline void gsl_interp_accel_free(gsl_interp_accel *a) { delete a; }

inline double gsl_interp_eval(const gsl_interp *it, const double *xa, const double *ya, double x, gsl_interp_accel *a) {
    const size_t n = it->size;
    if (n < 2 || x <= xa[0]) return ya[0];
    if (x >= xa[n - 1]) return ya[n - 1];
    size_t lo = 0, hi = n - 1;  /* xa[lo] <= x < xa[hi] */
    if (a && a->cache + 1 < n && xa[a->cache] <= x && x < xa[a->cache + 1]) {
        lo = a->cache;
        hi = lo + 1;
    }
    while (hi - lo > 1) {
        const size_t mid = lo + (hi - lo) / 2;
        if (xa[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    if (a) a->cache = lo;
    const double dx = xa[lo + 1] - xa[lo];
    return dx > 0 ? ya[lo] + (x - xa[lo]) / dx * (ya[lo + 1] - ya[lo]) : ya[lo];
}
