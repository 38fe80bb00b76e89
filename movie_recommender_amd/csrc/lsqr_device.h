// Device side of the general sparse LSQR (lsqr.hip; include/mr_lsqr.h): the
// scalar state and the three last-workgroup rules, which restate
// scipy/sparse/linalg/_isolve/lsqr.py (1.15) operation for operation.
//
// The Golub-Kahan vectors are stored UNNORMALISED, uh = beta u and vh = alfa v,
// beside their scales us = 1 / beta and vs = 1 / alfa (1 where SciPy leaves
// the vector unscaled: a zero norm).  A kernel forms u_i = us * uh_i and v_j =
// vs * vh_j where it loads them -- SciPy's `(1/beta) * u` -- so no scaling
// pass runs.  Per iteration:
//   KA  uh_i = sum_j a_ij v_j - alfa u_i   (csr_spmv_kernel, kernels.hip)
//       last workgroup: lsqr_after_a -- beta, us, anorm
//   KT  vh_j = sum_i a_ij u_i - beta v_j   (skipped when beta == 0)
//       last workgroup: lsqr_after_t -- alfa, vs, both rotations, t1, t2,
//       1 / rho, the ||x|| estimate, rnorm, arnorm, r1norm
//   KX  dk = (1/rho) w, x += t1 w, w = v + t2 w   (lsqr_x_kernel, lsqr.hip)
//       last workgroup: lsqr_after_x -- ddnorm, acond, the seven stopping
//       tests in SciPy's order, publish
// Every norm is the sqrt of a fixed-order sum of squares (per thread, per
// workgroup, then the partials in index order); nothing is scaled against
// overflow.  fp contraction is off in every rule.
#pragma once
#include "mr_internal.h"

namespace mr {

struct LsqrState {
  double alfa, beta;
  double us, vs;   // scales of the stored uh / vh
  double rhobar, phibar, anorm, acond, ddnorm, res2, xnorm, xxnorm, z, cs2, sn2;
  double rnorm, r1norm, r2norm, arnorm, bnorm;
  double damp, dampsq, atol, btol, ctol;
  double t1, t2, irho;   // KX's coefficients (phi / rho, -theta / rho, 1 / rho)
  int32_t itn, istop;
  int32_t done;          // solve finished: every later kernel is a no-op
  int32_t iter_lim;
  int32_t setup;         // 1 until the setup's KX has run
  int32_t skip_t;        // beta == 0: this iteration's KT leaves v and alfa
  int32_t bnorm_is_beta; // no x0: bnorm = the setup's beta (SciPy: bnorm.copy())
  uint32_t arrive;       // workgroups finished (the last one applies the rule)
};

// csr_spmv_kernel's lmode bits (LSQR_LSMR: the rules of lsmr_device.h)
enum LsqrMode { LSQR_KT = 1, LSQR_NEG = 2, LSQR_LSMR = 4 };

__device__ __forceinline__ double lsqr_sign(double a) {
  return a > 0.0 ? 1.0 : (a < 0.0 ? -1.0 : a);   // np.sign: 0 -> 0, nan -> nan
}

// _sym_ortho (lsqr.py:62-94), its zero cases included.
__device__ __forceinline__ void lsqr_sym_ortho(double a, double b, double& c, double& s,
                                               double& r) {
#pragma clang fp contract(off)
  if (b == 0.0) {
    c = lsqr_sign(a);
    s = 0.0;
    r = fabs(a);
  } else if (a == 0.0) {
    c = 0.0;
    s = lsqr_sign(b);
    r = fabs(b);
  } else if (fabs(b) > fabs(a)) {
    const double tau = a / b;
    s = lsqr_sign(b) / sqrt(1.0 + tau * tau);
    c = s * tau;
    r = b / s;
  } else {
    const double tau = b / a;
    c = lsqr_sign(a) / sqrt(1.0 + tau * tau);
    s = c * tau;
    r = a / c;
  }
}

// KA's rule on tot = sum uh_i^2 (lsqr.py:382-385 in the setup, :431-435).
__device__ __forceinline__ void lsqr_after_a(LsqrState* st, double tot) {
#pragma clang fp contract(off)
  const double beta = sqrt(tot);
  st->beta = beta;
  st->us = beta > 0.0 ? 1.0 / beta : 1.0;
  if (st->setup) {
    if (st->bnorm_is_beta) st->bnorm = beta;
    return;
  }
  st->itn += 1;
  st->skip_t = beta > 0.0 ? 0 : 1;
  if (beta > 0.0) {
    const double an = st->anorm, al = st->alfa;
    st->anorm = sqrt(an * an + al * al + beta * beta + st->dampsq);
  }
}

// KT's rule on tot = sum vh_j^2: alfa (lsqr.py:387-400 in the setup,
// :437-439), then the scalar recurrence of the iteration (:443-513).
__device__ __forceinline__ void lsqr_after_t(LsqrState* st, double tot) {
#pragma clang fp contract(off)
  const double beta = st->beta;
  if (st->setup) {
    const double alfa = sqrt(tot);
    st->alfa = alfa;
    st->vs = alfa > 0.0 ? 1.0 / alfa : 1.0;
    st->rhobar = alfa;
    st->phibar = beta;
    st->rnorm = st->r1norm = st->r2norm = beta;
    st->arnorm = alfa * beta;
    return;
  }
  double alfa = st->alfa;
  if (!st->skip_t) {
    alfa = sqrt(tot);
    st->alfa = alfa;
    st->vs = alfa > 0.0 ? 1.0 / alfa : 1.0;
  }
  const double damp = st->damp, dampsq = st->dampsq;
  double rhobar = st->rhobar, phibar = st->phibar;
  double rhobar1, psi;
  if (damp > 0.0) {
    rhobar1 = sqrt(rhobar * rhobar + dampsq);
    const double cs1 = rhobar / rhobar1;
    const double sn1 = damp / rhobar1;
    psi = sn1 * phibar;
    phibar = cs1 * phibar;
  } else {
    rhobar1 = rhobar;
    psi = 0.0;
  }
  double cs, sn, rho;
  lsqr_sym_ortho(rhobar1, beta, cs, sn, rho);
  const double theta = sn * alfa;
  rhobar = -cs * alfa;
  const double phi = cs * phibar;
  phibar = sn * phibar;
  const double tau = sn * phi;
  st->rhobar = rhobar;
  st->phibar = phibar;
  st->t1 = phi / rho;
  st->t2 = -theta / rho;
  st->irho = 1.0 / rho;
  // the rotation on the right and the estimate of norm(x)
  const double delta = st->sn2 * rho;
  const double gambar = -st->cs2 * rho;
  const double rhs = phi - delta * st->z;
  const double zbar = rhs / gambar;
  const double xxnorm0 = st->xxnorm;
  st->xnorm = sqrt(xxnorm0 + zbar * zbar);
  const double gamma = sqrt(gambar * gambar + theta * theta);
  st->cs2 = gambar / gamma;
  st->sn2 = theta / gamma;
  const double z = rhs / gamma;
  st->z = z;
  const double xxnorm = xxnorm0 + z * z;
  st->xxnorm = xxnorm;
  const double res1 = phibar * phibar;
  const double res2 = st->res2 + psi * psi;
  st->res2 = res2;
  const double rnorm = sqrt(res1 + res2);
  st->rnorm = rnorm;
  st->arnorm = alfa * fabs(tau);
  if (damp > 0.0) {
    const double r1sq = rnorm * rnorm - dampsq * xxnorm;
    double r1 = sqrt(fabs(r1sq));
    if (r1sq < 0.0) r1 = -r1;
    st->r1norm = r1;
  } else {
    st->r1norm = rnorm;
  }
  st->r2norm = rnorm;
}

// Seqlock publish into slot seq % kMirrorSlots of the host-mapped ring
// (wait_published): it = itn, ret = istop, rr = rnorm, final_rr = arnorm.
__device__ __forceinline__ void lsqr_publish(const LsqrState* st, CgMirror* ring, int seq) {
  CgMirror* m = ring + (seq & (kMirrorSlots - 1));
  __hip_atomic_store(&m->seq, 2 * seq - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();
  m->done = st->done;
  m->fails = 0;
  m->it = st->itn;
  m->ret = st->istop;
  m->n_matvec = st->itn;
  m->rr = st->rnorm;
  m->final_rr = st->arnorm;
  __threadfence_system();
  __hip_atomic_store(&m->seq, 2 * seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// KX's rule on tot = sum dk_j^2 (lsqr.py:471, :493, :517-543, :571): the
// setup's KX (w = v, tot unused) ends the setup -- arnorm == 0 returns at
// once (:405-408), iter_lim <= 0 never enters the loop.
__device__ __forceinline__ void lsqr_after_x(LsqrState* st, double tot, CgMirror* ring, int seq) {
#pragma clang fp contract(off)
  if (st->setup) {
    st->setup = 0;
    if (st->arnorm == 0.0 || st->iter_lim <= 0) st->done = 1;
    lsqr_publish(st, ring, seq);
    return;
  }
  const double eps = 2.220446049250313e-16;
  const double dn = sqrt(tot);
  const double ddnorm = st->ddnorm + dn * dn;
  st->ddnorm = ddnorm;
  const double anorm = st->anorm, rnorm = st->rnorm, xnorm = st->xnorm, bnorm = st->bnorm;
  const double acond = anorm * sqrt(ddnorm);
  st->acond = acond;
  const double test1 = rnorm / bnorm;
  const double test2 = st->arnorm / (anorm * rnorm + eps);
  const double test3 = 1.0 / (acond + eps);
  const double t1 = test1 / (1.0 + anorm * xnorm / bnorm);
  const double rtol = st->btol + st->atol * anorm * xnorm / bnorm;
  int istop = 0;
  if (st->itn >= st->iter_lim) istop = 7;
  if (1.0 + test3 <= 1.0) istop = 6;
  if (1.0 + test2 <= 1.0) istop = 5;
  if (1.0 + t1 <= 1.0) istop = 4;
  if (test3 <= st->ctol) istop = 3;
  if (test2 <= st->atol) istop = 2;
  if (test1 <= rtol) istop = 1;
  st->istop = istop;
  if (istop != 0) st->done = 1;
  lsqr_publish(st, ring, seq);
}

// Sum over a 256-thread workgroup in a fixed order (lanes by a xor butterfly,
// the four waves in wave order); valid on thread 0.  sh: 4 doubles.
__device__ __forceinline__ double lsqr_block_sum(double v, double* sh) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) t = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  return t;
}

// Every workgroup stores its sum; the one that arrives last adds the partials
// in index order and applies `rule(total)` on its thread 0.
template <class Rule>
__device__ __forceinline__ void lsqr_last_block(LsqrState* st, double* partials, double tot,
                                                double* sh, Rule&& rule) {
  __shared__ int s_last;
  if (threadIdx.x == 0) {
    __hip_atomic_store(&partials[blockIdx.x], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_last = __hip_atomic_fetch_add(&st->arrive, 1u, __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  double acc = 0.0;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x)
    acc += __hip_atomic_load(&partials[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const double total = lsqr_block_sum(acc, sh);
  if (threadIdx.x == 0) {
    __hip_atomic_store(&st->arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    rule(total);
  }
}

}  // namespace mr
