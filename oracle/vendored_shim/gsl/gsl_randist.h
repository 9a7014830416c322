/* Names only; see gsl_rng.h. */
#pragma once
#include "gsl_rng.h"
double gsl_ran_gaussian(gsl_rng *, double);
double gsl_ran_gaussian_ziggurat(gsl_rng *, double);
double gsl_ran_rayleigh(gsl_rng *, double);
void gsl_ran_shuffle(gsl_rng *, void *, size_t, size_t);
