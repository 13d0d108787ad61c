/* Reference for the per-residue posterior probabilities of an alignment path (tests/pp_reference.py builds and calls
 * this file; TEST INFRASTRUCTURE ONLY).
 *
 * Unihit-local Forward / Backward / posterior decoding with the recurrences, the row rescaling and the length model of
 * oracle/p7_oracle.c (forward_x / backward_x / len_config), on the configured profile the oracle exposes (pt, odds,
 * entry).  Like the oracle's hmmalign restatement it runs in x87 long double: with row rescaling alone a scaled double
 * does not hold a query with two copies of a long family (the N state falls below its range behind the first copy),
 * and those are the pairs the device redoes in log space.  On everything else long double only adds digits.
 *
 * Nothing is kept but the cells of the given path: each sweep walks the rows once with two rolling rows and picks, per
 * residue i, the cell of the state the path puts it in (st: 0 M_k, 1 I_k, 2 N, 3 C):
 *     M_k: F_M(i,k) B_M(i,k) / Z      I_k: F_I(i,k) B_I(i,k) / Z
 *     N:   F_N(i-1) loop B_N(i) / Z   C:   F_C(i-1) loop B_C(i) / Z
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

enum { tMM = 0, tMI = 1, tMD = 2, tIM = 3, tII = 4, tDM = 5, tDD = 6 };
#define RESCALE_HI 1e60L

/* pt [M+1][7], odds [Kp][M+1], entry [M+2]; loop / move: the float32 ploop / pmove of the caller; st / kk [L];
 * out [L].  Returns 0, or 1 when no alignment has probability (out = 0). */
int ppref_path(int M, const double *pt, const double *odds, const double *entry, const uint8_t *dsq, int L, double loop,
               double move, const int *st, const int *kk, double *out)
{
  const size_t W = (size_t) M + 2;
  long double *buf = (long double *) calloc(6 * W + 4 * ((size_t) L + 1), sizeof(long double));
  long double *pm = buf, *pi = pm + W, *pd = pi + W, *cm = pd + W, *ci = cm + W, *cd = ci + W;
  long double *fcell = cd + W, *fN = fcell + L + 1, *fC = fN + L + 1, *lsF = fC + L + 1;
  long double xN = 1.0L, xC = 0.0L, xB = move, ls = 0.0L, fwd;
  int i, k;
  for (i = 0; i < L; i++) out[i] = 0.0;
  if (!buf || L <= 0) { free(buf); return 1; }
  /* ---------------- Forward */
  fN[0] = 1.0L; fC[0] = 0.0L; lsF[0] = 0.0L;
  for (i = 1; i <= L; i++) {
    const double *od = odds + (size_t) dsq[i - 1] * (M + 1);
    long double xE = 0.0L, *t;
    cm[0] = ci[0] = cd[0] = 0.0L;
    for (k = 1; k <= M; k++) {
      const double *tp = pt + (size_t) (k - 1) * 7, *tk = pt + (size_t) k * 7;
      const long double m = od[k] * (pm[k - 1] * tp[tMM] + pi[k - 1] * tp[tIM] + pd[k - 1] * tp[tDM] + xB * entry[k]);
      const long double d = cm[k - 1] * tp[tMD] + cd[k - 1] * tp[tDD];
      const long double ins = pm[k] * tk[tMI] + pi[k] * tk[tII];
      cm[k] = m; ci[k] = ins; cd[k] = d;
      xE += m + d;
    }
    xN = xN * loop;
    xC = xC * loop + xE;
    if (xE > RESCALE_HI) {
      const long double r = 1.0L / xE;
      for (k = 1; k <= M; k++) { cm[k] *= r; ci[k] *= r; cd[k] *= r; }
      xN *= r; xC *= r; ls += logl(xE);
    }
    xB = xN * move;
    fN[i] = xN; fC[i] = xC; lsF[i] = ls;
    fcell[i] = st[i - 1] == 0 ? cm[kk[i - 1]] : st[i - 1] == 1 ? ci[kk[i - 1]] : 0.0L;
    t = pm; pm = cm; cm = t; t = pi; pi = ci; ci = t; t = pd; pd = cd; cd = t;
  }
  if (!(xC > 0.0L)) { free(buf); return 1; }
  fwd = ls + logl(xC * move);
  /* ---------------- Backward; pm / pi / pd = row i + 1 */
  {
    long double nN = 0.0L, nC = 0.0L;
    ls = 0.0L;
    for (k = 0; k <= M + 1; k++) { pm[k] = pi[k] = pd[k] = 0.0L; }
    for (i = L; i >= 1; i--) {
      const double *od = i < L ? odds + (size_t) dsq[i] * (M + 1) : NULL;    /* residue x_{i+1} */
      long double xBv = 0.0L, xNv, xCv, xE, p, *t;
      if (i == L) { xCv = move; xNv = 0.0L; }
      else {
        for (k = 1; k <= M; k++) xBv += pm[k] * od[k] * entry[k];
        xCv = nC * loop;
        xNv = nN * loop + xBv * move;
      }
      xE = xCv;
      cm[M] = xE; cd[M] = xE; ci[M] = 0.0L;
      for (k = M - 1; k >= 1; k--) {
        const double *tk = pt + (size_t) k * 7;
        const long double mnext = i < L ? pm[k + 1] * od[k + 1] : 0.0L;
        cm[k] = mnext * tk[tMM] + pi[k] * tk[tMI] + cd[k + 1] * tk[tMD] + xE;
        ci[k] = mnext * tk[tIM] + pi[k] * tk[tII];
        cd[k] = mnext * tk[tDM] + cd[k + 1] * tk[tDD] + xE;
      }
      if (xBv > RESCALE_HI || xNv > RESCALE_HI) {
        const long double big = xBv > xNv ? xBv : xNv, r = 1.0L / big;
        for (k = 1; k <= M; k++) { cm[k] *= r; ci[k] *= r; cd[k] *= r; }
        xCv *= r; xNv *= r; ls += logl(big);
      }
      switch (st[i - 1]) {
        case 0:  p = fcell[i] * cm[kk[i - 1]] * expl(lsF[i] + ls - fwd); break;
        case 1:  p = fcell[i] * ci[kk[i - 1]] * expl(lsF[i] + ls - fwd); break;
        case 2:  p = fN[i - 1] * loop * xNv * expl(lsF[i - 1] + ls - fwd); break;
        default: p = fC[i - 1] * loop * xCv * expl(lsF[i - 1] + ls - fwd); break;
      }
      out[i - 1] = (double) p;
      nN = xNv; nC = xCv;
      t = pm; pm = cm; cm = t; t = pi; pi = ci; ci = t; t = pd; pd = cd; cd = t;
    }
  }
  free(buf);
  return 0;
}
