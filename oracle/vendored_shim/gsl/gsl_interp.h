/* Names only; see gsl_rng.h. */
#pragma once
typedef struct gsl_interp gsl_interp;
typedef struct gsl_interp_accel gsl_interp_accel;
