// Device side of the sparse LSMR (lsqr.hip; mr_lsqr_solve_lsmr in
// include/mr_lsqr.h): the scalar state and the three last-workgroup rules,
// which restate scipy/sparse/linalg/_isolve/lsmr.py (1.15) operation for
// operation.
//
// LSMR runs on LSQR's Golub-Kahan process, so KA and KT are LSQR's passes
// (lsqr_device.h: uh, vh unnormalised beside us, vs; SciPy's `u *= -alpha;
// u += A v` is LSQR's `A v - alfa u` to the bit).  The LSMR state starts with
// an LsqrState: the passes read (alfa, us, vs, beta, skip_t, done, arrive)
// from it exactly as in an LSQR solve, the bnorm kernel writes normb into its
// bnorm, and itn / istop / done / iter_lim / setup / the tolerances / damp
// live there too.  Under the LSQR_LSMR bit of lmode the last workgroup's
// thread 0 applies the rules below instead of LSQR's.  Per iteration:
//   KA  lsmr_after_a -- beta, us, normA2 += beta^2, normA
//   KT  lsmr_after_t -- alpha, vs, the three rotations, zeta, zetabar, the
//       ||r|| estimate, normA2 += alpha^2, condA, normar, KX's coefficients
//   KX  hbar = hbar ch + h, x += cx hbar, h = h chh + v   (lsmr_x_kernel)
//       lsmr_after_x -- normx = ||x||, the seven stopping tests, publish
#pragma once
#include "lsqr_device.h"

namespace mr {

struct LsmrState {
  LsqrState q;   // first: the SpMV passes and lsqr_last_block see an LsqrState
  double zetabar, alphabar, rho, rhobar, cbar, sbar;
  double betadd, betad, rhodold, tautildeold, thetatilde, zeta, d;
  double normA2, maxrbar, minrbar;
  double normA, condA, normx, normr, normar;
  double ch, cx, chh;   // KX's coefficients
  int32_t zero_x;       // normb == 0 past the setup: SciPy returns x[()] = 0
  int32_t pad_;
};

// KA's rule on tot = sum uh_i^2 (lsmr.py:237-245 in the setup, :328-330, :399-400).
__device__ __forceinline__ void lsmr_after_a(LsmrState* st, double tot) {
#pragma clang fp contract(off)
  LsqrState* q = &st->q;
  const double beta = sqrt(tot);
  q->beta = beta;
  q->us = beta > 0.0 ? 1.0 / beta : 1.0;
  if (q->setup) {
    if (q->bnorm_is_beta) q->bnorm = beta;
    return;
  }
  q->itn += 1;
  q->skip_t = beta > 0.0 ? 0 : 1;
  const double normA2 = st->normA2 + beta * beta;
  st->normA2 = normA2;
  st->normA = sqrt(normA2);
}

// KT's rule on tot = sum vh_j^2: the setup (lsmr.py:247-299), or alpha
// (:332-338) and the scalar recurrence of the iteration (:344-412).
__device__ __forceinline__ void lsmr_after_t(LsmrState* st, double tot) {
#pragma clang fp contract(off)
  LsqrState* q = &st->q;
  const double beta = q->beta;
  if (q->setup) {
    const double alpha = sqrt(tot);
    q->alfa = alpha;
    q->vs = alpha > 0.0 ? 1.0 / alpha : 1.0;
    st->zetabar = alpha * beta;
    st->alphabar = alpha;
    st->rho = st->rhobar = st->cbar = 1.0;
    st->sbar = 0.0;
    st->betadd = beta;
    st->betad = 0.0;
    st->rhodold = 1.0;
    st->tautildeold = st->thetatilde = st->zeta = st->d = 0.0;
    const double normA2 = alpha * alpha;
    st->normA2 = normA2;
    st->maxrbar = 0.0;
    st->minrbar = 1e+100;
    st->normA = sqrt(normA2);
    st->condA = 1.0;
    st->normx = 0.0;
    st->normr = beta;
    st->normar = alpha * beta;
    return;
  }
  double alpha = q->alfa;
  if (!q->skip_t) {
    alpha = sqrt(tot);
    q->alfa = alpha;
    q->vs = alpha > 0.0 ? 1.0 / alpha : 1.0;
  }
  double chat, shat, alphahat;
  lsqr_sym_ortho(st->alphabar, q->damp, chat, shat, alphahat);
  const double rhoold = st->rho;
  double c, s, rho;
  lsqr_sym_ortho(alphahat, beta, c, s, rho);
  const double thetanew = s * alpha;
  st->alphabar = c * alpha;
  st->rho = rho;
  const double rhobarold = st->rhobar;
  const double zetaold = st->zeta;
  const double thetabar = st->sbar * rho;
  const double rhotemp = st->cbar * rho;
  double cbar, sbar, rhobar;
  lsqr_sym_ortho(st->cbar * rho, thetanew, cbar, sbar, rhobar);
  st->cbar = cbar;
  st->sbar = sbar;
  st->rhobar = rhobar;
  const double zeta = cbar * st->zetabar;
  const double zetabar = -sbar * st->zetabar;
  st->zeta = zeta;
  st->zetabar = zetabar;
  st->ch = -(thetabar * rho / (rhoold * rhobarold));
  st->cx = zeta / (rho * rhobar);
  st->chh = -(thetanew / rho);
  // the estimate of ||r||
  const double betaacute = chat * st->betadd;
  const double betacheck = -shat * st->betadd;
  const double betahat = c * betaacute;
  const double betadd = -s * betaacute;
  st->betadd = betadd;
  const double thetatildeold = st->thetatilde;
  double ctildeold, stildeold, rhotildeold;
  lsqr_sym_ortho(st->rhodold, thetabar, ctildeold, stildeold, rhotildeold);
  const double thetatilde = stildeold * rhobar;
  const double rhodold = ctildeold * rhobar;
  const double betad = -stildeold * st->betad + ctildeold * betahat;
  st->thetatilde = thetatilde;
  st->rhodold = rhodold;
  st->betad = betad;
  const double tautildeold = (zetaold - thetatildeold * st->tautildeold) / rhotildeold;
  st->tautildeold = tautildeold;
  const double taud = (zeta - thetatilde * tautildeold) / rhodold;
  const double d = st->d + betacheck * betacheck;
  st->d = d;
  const double bt = betad - taud;
  st->normr = sqrt(d + bt * bt + betadd * betadd);
  // ||A|| was taken in lsmr_after_a; cond(A)
  st->normA2 = st->normA2 + alpha * alpha;
  const double maxrbar = rhobarold > st->maxrbar ? rhobarold : st->maxrbar;   // Python's max(a, b)
  st->maxrbar = maxrbar;
  double minrbar = st->minrbar;
  if (q->itn > 1) {
    minrbar = rhobarold < minrbar ? rhobarold : minrbar;
    st->minrbar = minrbar;
  }
  st->condA = (rhotemp > maxrbar ? rhotemp : maxrbar) / (rhotemp < minrbar ? rhotemp : minrbar);
  st->normar = fabs(zetabar);
}

// KX's rule on tot = sum x_j^2 (lsmr.py:413-449).  The setup's KX (h = v,
// hbar = 0, tot unused) ends the setup: normar == 0 returns at once
// (:300-303), normb == 0 returns x = 0 (:305-307), maxiter <= 0 never enters
// the loop.
__device__ __forceinline__ void lsmr_after_x(LsmrState* st, double tot, CgMirror* ring, int seq) {
#pragma clang fp contract(off)
  LsqrState* q = &st->q;
  if (q->setup) {
    q->setup = 0;
    if (st->normar == 0.0) {
      q->done = 1;
    } else if (q->bnorm == 0.0) {
      q->done = 1;
      st->zero_x = 1;
    } else if (q->iter_lim <= 0) {
      q->done = 1;
    }
  } else {
    const double normx = sqrt(tot);
    st->normx = normx;
    const double normA = st->normA, normr = st->normr, normb = q->bnorm;
    const double test1 = normr / normb;
    const double an = normA * normr;
    const double test2 = an != 0.0 ? st->normar / an : __builtin_inf();
    const double test3 = 1.0 / st->condA;
    const double t1 = test1 / (1.0 + normA * normx / normb);
    const double rtol = q->btol + q->atol * normA * normx / normb;
    int istop = 0;
    if (q->itn >= q->iter_lim) istop = 7;
    if (1.0 + test3 <= 1.0) istop = 6;
    if (1.0 + test2 <= 1.0) istop = 5;
    if (1.0 + t1 <= 1.0) istop = 4;
    if (test3 <= q->ctol) istop = 3;
    if (test2 <= q->atol) istop = 2;
    if (test1 <= rtol) istop = 1;
    q->istop = istop;
    if (istop != 0) q->done = 1;
  }
  q->rnorm = st->normr;   // the ring's rr / final_rr
  q->arnorm = st->normar;
  lsqr_publish(q, ring, seq);
}

}  // namespace mr
