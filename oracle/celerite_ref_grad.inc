/*
 * oracle/celerite_ref_grad.inc -- forward-mode (tangent) gradient of the log-likelihood, the restatement of
 * celerite/solver.cpp:347-463 (the reference's AutoDiffScalar instantiation of compute + dot_solve) that
 * oracle/grad.py carries in Python, written once for a scalar type.  TEST INFRASTRUCTURE ONLY (see celerite_ref.h).
 *
 * Expects:  T          the scalar type (double, __float128)
 *           SUFFIX     name suffix
 *           T_EXP, T_LOG, T_COS, T_SIN   the type's elementary functions
 *
 * A "dual" here is L = 1 + K consecutive T values: the value, then the tangents along the K directions a worker
 * carries.  Every operation follows oracle/grad.py's Dual (value first, tangent formulas term for term, in the same
 * order), so that the double instantiation reproduces grad.py to rounding.  The tangent of one direction never reads
 * another direction's tangent: a direction's result does not depend on which others share its worker.
 */

#define CAT_(a, b) a##b
#define CAT(a, b) CAT_(a, b)
#define DUAL(name) CAT(name, SUFFIX)

/* o = a * b (o may alias a or b: the value is written last) */
static inline void DUAL(dmul_)(T* o, const T* a, const T* b, int L) {
  for (int k = 1; k < L; ++k) o[k] = a[k] * b[0] + a[0] * b[k];
  o[0] = a[0] * b[0];
}
/* o = a * c for a constant c */
static inline void DUAL(dmulc_)(T* o, const T* a, T c, int L) {
  for (int k = 0; k < L; ++k) o[k] = a[k] * c;
}
static inline void DUAL(dadd_)(T* o, const T* a, const T* b, int L) {
  for (int k = 0; k < L; ++k) o[k] = a[k] + b[k];
}
static inline void DUAL(dsub_)(T* o, const T* a, const T* b, int L) {
  for (int k = 0; k < L; ++k) o[k] = a[k] - b[k];
}
/* o = a / b: q = a / b, (a' - q b') / b */
static inline void DUAL(ddiv_)(T* o, const T* a, const T* b, int L) {
  const T q = a[0] / b[0], bv = b[0];
  for (int k = 1; k < L; ++k) o[k] = (a[k] - q * b[k]) / bv;
  o[0] = q;
}

typedef struct {
  /* problem */
  double jitter;
  int J_real, J_comp, J_general, N, compute_jitter, phase_in_double;
  const double *a_real, *c_real, *a_comp, *b_comp, *c_comp, *d_comp, *A, *U, *V, *t, *diag, *y;
  /* this worker's directions: K rows of G entries */
  int K, G;
  const double* dirs;
  /* out */
  double value;
  double* dval;
  int status;
} DUAL(grad_job_);

static void* DUAL(grad_worker_)(void* arg) {
  DUAL(grad_job_)* jb = (DUAL(grad_job_)*)arg;
  const int JR = jb->J_real, JC = jb->J_comp, JG = jb->J_general, N = jb->N, K = jb->K, G = jb->G;
  const int J = JR + 2 * JC + JG, L = 1 + K;
  const size_t Ls = (size_t)L;
  const int has_general = jb->A != NULL;
  /* duals: parameters (jitter, a_real, c_real, a_comp, b_comp, c_comp, d_comp), then the sweep's state */
  const int NP = 1 + 2 * JR + 4 * JC;
  const size_t n_duals = (size_t)NP + 3 * (size_t)J /* W_prev, Wn, f */ + (size_t)J * (size_t)J /* S */ +
                         2 * (size_t)J /* phi, u */ + 12 /* scalars */;
  T* mem = (T*)calloc(n_duals * Ls, sizeof(T));
  jb->status = REF_OK;
  if (!mem) { jb->status = REF_NO_MEMORY; return NULL; }
  T* par = mem;                                         /* par[p * L], p in the order of the gradient */
  T* Wp = par + (size_t)NP * Ls;
  T* Wn = Wp + (size_t)J * Ls;
  T* f = Wn + (size_t)J * Ls;
  T* S = f + (size_t)J * Ls;                            /* S[(k + J j) * L], k <= j */
  T* phi = S + (size_t)J * J * Ls;
  T* u = phi + (size_t)J * Ls;
  T* sc = u + (size_t)J * Ls;
  T *asum = sc, *csum = sc + Ls, *Dn = sc + 2 * Ls, *xm1 = sc + 3 * Ls, *res = sc + 4 * Ls, *logdet = sc + 5 * Ls,
    *tmp = sc + 6 * Ls, *tmp2 = sc + 7 * Ls, *xj = sc + 8 * Ls, *val = sc + 9 * Ls, *cd = sc + 10 * Ls, *sd = sc + 11 * Ls;
#define P_(p) (par + (size_t)(p) * Ls)
#define JIT P_(0)
#define AR(j) P_(1 + (j))
#define CR(j) P_(1 + JR + (j))
#define AC(j) P_(1 + 2 * JR + (j))
#define BC(j) P_(1 + 2 * JR + JC + (j))
#define CC(j) P_(1 + 2 * JR + 2 * JC + (j))
#define DC(j) P_(1 + 2 * JR + 3 * JC + (j))
  {
    const double* pv[7] = {&jb->jitter, jb->a_real, jb->c_real, jb->a_comp, jb->b_comp, jb->c_comp, jb->d_comp};
    const int pn[7] = {1, JR, JR, JC, JC, JC, JC};
    for (int g = 0, p = 0; g < 7; ++g)
      for (int i = 0; i < pn[g]; ++i, ++p) {
        T* q = P_(p);
        q[0] = (T)pv[g][i];
        for (int k = 0; k < K; ++k) q[1 + k] = (p == 0 && !jb->compute_jitter) ? (T)0 : (T)jb->dirs[(size_t)k * G + p];
      }
  }
  /* phase d t: the value fl(d t) in double when asked (what the reference and the device form), else the product
   * carried in T; its tangent is d' t either way */
#define PHASE(out, dj, tt)                                                              \
  do {                                                                                  \
    const double t_ = (tt);                                                             \
    (out)[0] = jb->phase_in_double ? (T)((double)(dj)[0] * t_) : (dj)[0] * (T)t_;       \
    for (int k_ = 1; k_ < L; ++k_) (out)[k_] = (dj)[k_] * (T)t_;                        \
  } while (0)
  /* cos / sin of a dual */
#define DCOS(out, x) do { const T s_ = T_SIN((x)[0]), c_ = T_COS((x)[0]); \
    for (int k_ = 1; k_ < L; ++k_) { (out)[k_] = -s_ * (x)[k_]; } (out)[0] = c_; } while (0)
#define DSIN(out, x) do { const T s_ = T_SIN((x)[0]), c_ = T_COS((x)[0]); \
    for (int k_ = 1; k_ < L; ++k_) { (out)[k_] = c_ * (x)[k_]; } (out)[0] = s_; } while (0)
  /* D_n before the update: ((diag + sum a_real) + sum a_comp) + jitter (+ A) */
#define DBASE(out, n) do { for (int k_ = 0; k_ < L; ++k_) (out)[k_] = (asum[k_] + csum[k_]) + JIT[k_]; \
    (out)[0] = (((T)jb->diag[n] + asum[0]) + csum[0]) + JIT[0];                                          \
    if (has_general) (out)[0] = (out)[0] + (T)jb->A[n]; } while (0)

  for (int j = 0; j < JR; ++j) DUAL(dadd_)(asum, asum, AR(j), L);   /* zero + a_0 + a_1 ... */
  for (int j = 0; j < JC; ++j) DUAL(dadd_)(csum, csum, AC(j), L);
  /* tangent of ((diag + asum) + csum) + jit: the constant diag adds nothing; (asum' + csum') + jit' */
  DBASE(Dn, 0);
  /* log det and the quadratic form: cholesky.h:98-117 at n = 0, :347 */
  {
    for (int k = 0; k < L; ++k) val[k] = 0;
    val[0] = 1;
    DUAL(ddiv_)(val, val, Dn, L);                                   /* value = 1 / D_0 */
    const double t0 = jb->t[0];
    for (int j = 0; j < JR; ++j) memcpy(Wp + (size_t)j * Ls, val, Ls * sizeof(T));
    for (int j = 0, k = JR; j < JC; ++j, k += 2) {
      PHASE(tmp, DC(j), t0);
      DCOS(cd, tmp);
      DSIN(sd, tmp);
      DUAL(dmul_)(Wp + (size_t)k * Ls, cd, val, L);
      DUAL(dmul_)(Wp + (size_t)(k + 1) * Ls, sd, val, L);
    }
    for (int j = 0, k = JR + 2 * JC; j < JG; ++j, ++k) DUAL(dmulc_)(Wp + (size_t)k * Ls, val, (T)jb->V[(size_t)j * N], L);
    for (int k = 0; k < L; ++k) xm1[k] = 0;
    xm1[0] = (T)jb->y[0];
    DUAL(ddiv_)(tmp, xm1, Dn, L);
    DUAL(dmul_)(res, xm1, tmp, L);
    /* log det accumulates log D_n in n order */
    for (int k = 1; k < L; ++k) logdet[k] = logdet[k] + Dn[k] / Dn[0];
    logdet[0] = logdet[0] + T_LOG(Dn[0]);
  }

  for (int n = 1; n < N; ++n) {                                     /* cholesky.h:126-179 */
    const double tn = jb->t[n];
    const T dx = (T)tn - (T)jb->t[n - 1];
    for (int j = 0; j < JR; ++j) {                                  /* :129-133 */
      T* ph = phi + (size_t)j * Ls;
      for (int k = 0; k < L; ++k) ph[k] = -CR(j)[k] * dx;
      const T e = T_EXP(ph[0]);
      for (int k = 1; k < L; ++k) ph[k] = e * ph[k];
      ph[0] = e;
      memcpy(u + (size_t)j * Ls, AR(j), Ls * sizeof(T));
      T* w = Wn + (size_t)j * Ls;
      for (int k = 0; k < L; ++k) w[k] = 0;
      w[0] = 1;
    }
    for (int j = 0, k = JR; j < JC; ++j, k += 2) {                  /* :134-147 */
      PHASE(tmp, DC(j), tn);
      DCOS(cd, tmp);
      DSIN(sd, tmp);
      T* ph = phi + (size_t)k * Ls;
      for (int q = 0; q < L; ++q) ph[q] = -CC(j)[q] * dx;
      const T e = T_EXP(ph[0]);
      for (int q = 1; q < L; ++q) ph[q] = e * ph[q];
      ph[0] = e;
      memcpy(phi + (size_t)(k + 1) * Ls, ph, Ls * sizeof(T));
      DUAL(dmul_)(tmp, AC(j), cd, L);
      DUAL(dmul_)(tmp2, BC(j), sd, L);
      DUAL(dadd_)(u + (size_t)k * Ls, tmp, tmp2, L);                /* a cos + b sin */
      DUAL(dmul_)(tmp, AC(j), sd, L);
      DUAL(dmul_)(tmp2, BC(j), cd, L);
      DUAL(dsub_)(u + (size_t)(k + 1) * Ls, tmp, tmp2, L);          /* a sin - b cos */
      memcpy(Wn + (size_t)k * Ls, cd, Ls * sizeof(T));
      memcpy(Wn + (size_t)(k + 1) * Ls, sd, Ls * sizeof(T));
    }
    for (int j = 0, k = JR + 2 * JC; j < JG; ++j, ++k) {            /* :148-152 */
      T *ph = phi + (size_t)k * Ls, *uu = u + (size_t)k * Ls, *w = Wn + (size_t)k * Ls;
      for (int q = 0; q < L; ++q) ph[q] = uu[q] = w[q] = 0;
      ph[0] = 1;
      uu[0] = (T)jb->U[(size_t)j * N + n];
      w[0] = (T)jb->V[(size_t)j * N + n];
    }

    for (int j = 0; j < J; ++j) {                                   /* :154-160 */
      const T* phj = phi + (size_t)j * Ls;
      DUAL(dmul_)(xj, Dn, Wp + (size_t)j * Ls, L);
      for (int k = 0; k <= j; ++k) {
        T* s = S + ((size_t)k + (size_t)J * j) * Ls;
        DUAL(dmul_)(tmp, xj, Wp + (size_t)k * Ls, L);
        DUAL(dadd_)(tmp, s, tmp, L);
        DUAL(dmul_)(tmp, phi + (size_t)k * Ls, tmp, L);
        DUAL(dmul_)(s, phj, tmp, L);
      }
    }

    DBASE(Dn, n);                                                   /* :162-175 */
    for (int j = 0; j < J; ++j) {
      const T* uj = u + (size_t)j * Ls;
      memcpy(xj, Wn + (size_t)j * Ls, Ls * sizeof(T));
      for (int k = 0; k < j; ++k) {
        const T* s = S + ((size_t)k + (size_t)J * j) * Ls;
        DUAL(dmul_)(tmp, u + (size_t)k * Ls, s, L);
        DUAL(dmul_)(tmp2, uj, tmp, L);
        DUAL(dmulc_)(tmp2, tmp2, (T)2, L);
        DUAL(dsub_)(Dn, Dn, tmp2, L);
        DUAL(dsub_)(xj, xj, tmp, L);
        DUAL(dmul_)(tmp2, uj, s, L);
        DUAL(dsub_)(Wn + (size_t)k * Ls, Wn + (size_t)k * Ls, tmp2, L);
      }
      DUAL(dmul_)(tmp, uj, S + ((size_t)j + (size_t)J * j) * Ls, L);
      DUAL(dmul_)(tmp2, uj, tmp, L);
      DUAL(dsub_)(Dn, Dn, tmp2, L);
      DUAL(dsub_)(Wn + (size_t)j * Ls, xj, tmp, L);
    }
    if (Dn[0] < 0) { jb->status = REF_LINALG; break; }            /* :176 */
    for (int j = 0; j < J; ++j) DUAL(ddiv_)(Wn + (size_t)j * Ls, Wn + (size_t)j * Ls, Dn, L);  /* :178 */

    /* dot_solve, cholesky.h:348-357, in the same sweep (it only looks back) */
    for (int k = 0; k < L; ++k) val[k] = 0;
    val[0] = (T)jb->y[n];
    for (int j = 0; j < J; ++j) {
      T* fj = f + (size_t)j * Ls;
      DUAL(dmul_)(tmp, Wp + (size_t)j * Ls, xm1, L);
      DUAL(dadd_)(tmp, fj, tmp, L);
      DUAL(dmul_)(fj, phi + (size_t)j * Ls, tmp, L);
      DUAL(dmul_)(tmp, u + (size_t)j * Ls, fj, L);
      DUAL(dsub_)(val, val, tmp, L);
    }
    memcpy(xm1, val, Ls * sizeof(T));
    DUAL(dmul_)(tmp, val, val, L);
    DUAL(ddiv_)(tmp, tmp, Dn, L);
    DUAL(dadd_)(res, res, tmp, L);
    for (int k = 1; k < L; ++k) logdet[k] = logdet[k] + Dn[k] / Dn[0];
    logdet[0] = logdet[0] + T_LOG(Dn[0]);
    { T* sw = Wp; Wp = Wn; Wn = sw; }
  }
  if (jb->status == REF_OK) {
    /* solver.cpp:415: -0.5 (quad + log det + pi log N), the constant formed in double as the reference forms it */
    const T c = (T)(M_PI_ * log((double)N));
    jb->value = (double)((T)-0.5 * ((res[0] + logdet[0]) + c));
    for (int k = 0; k < K; ++k) jb->dval[k] = (double)((T)-0.5 * (res[1 + k] + logdet[1 + k]));
  }
  free(mem);
  return NULL;
#undef P_
#undef JIT
#undef AR
#undef CR
#undef AC
#undef BC
#undef CC
#undef DC
#undef PHASE
#undef DCOS
#undef DSIN
#undef DBASE
}

/* The value and ndir directional derivatives of the log-likelihood.  dirs: ndir x G row-major, G = 1 + 2 J_real +
 * 4 J_comp in the gradient's order (jitter, a_real, c_real, a_comp, b_comp, c_comp, d_comp); the jitter component
 * counts only when jitter > DBL_EPSILON (solver.cpp:379-389).  U, V row-major [J_general][N]; A NULL = no general
 * terms.  The directions are split over nthreads workers, each running the value sweep with its share of tangents:
 * the results do not depend on the thread count.  Returns REF_LINALG where the reference throws (cholesky.h:176). */
int CAT(ref_grad_, SUFFIX)(double jitter, int J_real, const double* a_real, const double* c_real,
                           int J_comp, const double* a_comp, const double* b_comp, const double* c_comp, const double* d_comp,
                           int J_general, const double* A, const double* U, const double* V,
                           int N, const double* t, const double* diag, const double* y,
                           int ndir, const double* dirs, int nthreads, int phase_in_double,
                           double* value, double* dval)
{
  if (N < 1 || J_real < 0 || J_comp < 0 || J_general < 0 || ndir < 0 || (J_general > 0 && (!A || !U || !V)))
    return REF_DIMENSION_MISMATCH;
  const int G = 1 + 2 * J_real + 4 * J_comp;
  if (nthreads < 1) nthreads = 1;
  if (nthreads > 64) nthreads = 64;
  if (nthreads > ndir) nthreads = ndir > 0 ? ndir : 1;
  DUAL(grad_job_) jobs[64];
  pthread_t th[64];
  const int per = ndir > 0 ? (ndir + nthreads - 1) / nthreads : 0;
  int nj = 0;
  for (int i = 0; i < nthreads; ++i) {
    const int d0 = i * per, d1 = (d0 + per < ndir) ? d0 + per : ndir;
    if (i > 0 && d0 >= ndir) break;
    DUAL(grad_job_)* jb = &jobs[nj++];
    memset(jb, 0, sizeof(*jb));
    jb->jitter = jitter;
    jb->J_real = J_real; jb->J_comp = J_comp; jb->J_general = J_general; jb->N = N;
    jb->compute_jitter = jitter > DBL_EPSILON_;
    jb->phase_in_double = phase_in_double;
    jb->a_real = a_real; jb->c_real = c_real; jb->a_comp = a_comp; jb->b_comp = b_comp;
    jb->c_comp = c_comp; jb->d_comp = d_comp;
    jb->A = J_general > 0 ? A : NULL; jb->U = U; jb->V = V;
    jb->t = t; jb->diag = diag; jb->y = y;
    jb->K = d1 > d0 ? d1 - d0 : 0;
    jb->G = G;
    jb->dirs = dirs + (size_t)d0 * G;
    jb->dval = dval + d0;
  }
  if (nj == 1) DUAL(grad_worker_)(&jobs[0]);
  else {
    for (int i = 0; i < nj; ++i) pthread_create(&th[i], NULL, DUAL(grad_worker_), &jobs[i]);
    for (int i = 0; i < nj; ++i) pthread_join(th[i], NULL);
  }
  for (int i = 0; i < nj; ++i)
    if (jobs[i].status != REF_OK) return jobs[i].status;
  if (value) *value = jobs[0].value;
  return REF_OK;
}

#undef DUAL
#undef CAT
#undef CAT_
