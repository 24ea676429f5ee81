/*
 * oracle/celerite_ref_grad.c -- the forward-mode gradient of celerite_ref_grad.inc instantiated for double (the twin
 * of oracle/grad.py, at C speed) and for IEEE binary128 (__float128, libquadmath: "the truth" the GPU gradient tests
 * attribute deviations with).  TEST INFRASTRUCTURE ONLY (see celerite_ref.h).
 *
 * Pinning: tests/test_oracle.py checks the double instantiation against oracle/grad.py per partial, the binary128 one
 * against an mpmath dense analytic gradient (oracle/dense.py), linearity in the direction and independence of the
 * thread count.
 */
#include <math.h>
#include <pthread.h>
#include <quadmath.h>
#include <stdlib.h>
#include <string.h>

#include "celerite_ref.h"

#define M_PI_ 3.14159265358979323846
#define DBL_EPSILON_ 2.220446049250313e-16

#define T double
#define SUFFIX d
#define T_EXP exp
#define T_LOG log
#define T_COS cos
#define T_SIN sin
#include "celerite_ref_grad.inc"
#undef T
#undef SUFFIX
#undef T_EXP
#undef T_LOG
#undef T_COS
#undef T_SIN

#define T __float128
#define SUFFIX q
#define T_EXP expq
#define T_LOG logq
#define T_COS cosq
#define T_SIN sinq
#include "celerite_ref_grad.inc"
