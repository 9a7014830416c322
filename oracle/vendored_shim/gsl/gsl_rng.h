/* Names only: the vendored library's channel simulator refers to these; none is on the
 * encode / decode path, and polar_ref links no GSL (see oracle/polar_ref.cpp). */
#pragma once
typedef struct gsl_rng gsl_rng;
typedef struct gsl_rng_type gsl_rng_type;
extern const gsl_rng_type *gsl_rng_mt19937;
extern const gsl_rng_type *gsl_rng_default;
gsl_rng *gsl_rng_alloc(const gsl_rng_type *);
void gsl_rng_free(gsl_rng *);
void gsl_rng_set(gsl_rng *, unsigned long);
unsigned long gsl_rng_get(gsl_rng *);
double gsl_rng_uniform(gsl_rng *);
unsigned long gsl_rng_uniform_int(gsl_rng *, unsigned long);
