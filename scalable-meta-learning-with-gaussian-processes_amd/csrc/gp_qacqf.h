// gp_qacqf.h -- the joint Monte-Carlo acquisition of a q-batch, qEI / qUCB, and its exact input gradient in one launch
// (include/scaml_gp.h (7p)): argument block, LDS footprint and the arithmetic of one batch.  One source for the device kernel
// (csrc/gp_qacqf.hip: a workgroup of 256 threads per batch), the host launcher and the single-threaded host build the CPU tests check
// against torch autograd (any compiler but hipcc: tests/host_emul/qacqf_emul.cpp).
//
// One batch is X = (x_1 .. x_q).  With the target GP's value path (Knq, Z = Knn^-1 Knq, alpha, mean_q, var_q; standardiser m, s) and the
// weighted sums of the joint GRAD pass (5g) -- rows a < n of cov_g against the training points, rows n + r against batch mate r --:
//   mu_j  = m + s (mean_q[j] + Knq[:, j] . alpha)
//   S_jk  = P_jk - Knq[:, j] . Z[:, k],   P_jj = var_q[j],   P_jk = cov_g[n + k][16 j] / s^2 + os k_t(x_j, x_k),   Sigma = s^2 S
//   C C^T = Sigma + jitter I   (ladder 0, 1e-8, 1e-7, 1e-6; an attempt fails on a pivot that is <= 0 or not finite)
//   f_s   = mu + C eps_s,      value = (1/S) sum_s a_s
//   qEI:  a_s = max_j max(best_f - f_sj, 0)            qUCB:  a_s = max_j (-mu_j + sqrt(beta pi / 2) |(C eps_s)_j|)
// (minimisation convention).  Sub-gradients: the arg-max is the lowest j that attains the maximum; max(., 0) and |.| have slope 0 at 0.
// Adjoint: mubar, Cbar summed over the samples; Phi = tril(C^T Cbar) with its diagonal halved; Sigmabar = sym(C^-T Phi C^-1).  Then, with
// mbar = s mubar and Sbar = s^2 Sigmabar, the gradient of point j is
//   mbar_j dmean_q[j] + Sbar_jj dvar_q[j] + 2 sum_{k != j} Sbar_jk dP_jk + sum_a dKnq[a][j] (mbar_j alpha_a - 2 sum_k Sbar_jk Z[a][k])
// -- the sum over the training points is contracted once per query point against ONE weight vector, as (7f) does with its abar.
//
// The q x q work lives in LDS and is done by the threads of the workgroup together (a per-thread q x q array indexed by a run-time q
// would sit in scratch memory).  The samples are dealt to the threads; what a sample adds to mubar, Cbar and the value is recorded in
// LDS and summed by ONE thread per entry over four fixed chunks of the sample axis, ascending: no atomics, no cross-wave reduction, so
// the result is a pure function of the inputs, whatever the number of threads, and the host build computes what the device computes.
//
// With p evaluations pending ((7q), qa_batch<true>) the joint vector is the q moving points followed by the p pending ones, Q = q + p,
// the same pending points in every batch.  They are LEADING points of (5g) (rows n + k of cov_g, in front of the mates' rows n + p + r), so
//   S_{j, q+k} = cov_g[n + k][16 j] / s^2 + os k_t(x_j, xp_k) - Knq[:, j] . Zp[:, k]     (Zp = Knn^-1 Knp),    Sigma = s^2 S
// and the pending block of Sigma and mu is given (Sigma_pp, mu_p: they do not depend on the batch).  The tail runs at Q; a pending point
// is held fixed, so the gradient of moving point j gains 2 sum_k Sbar_{j,q+k} dP_{j,q+k}/dx_j and its weight vector on dKnq[:, j] the
// term -2 sum_k Sbar_{j,q+k} Zp[:, k].  The pending rows of mbar and Sbar are not read.
//
// Value only ((7r), qa_batch<true, true>): the same joint posterior, ladder, samples and sums -- value, jitter and info are (7p)'s /
// (7q)'s bit for bit given the same numbers -- read from the VALUE layout of (5h): the B batches packed into Mp columns
// (csrc/gp_qacqf_columns.h; the points of a batch are consecutive columns), Knq, Z (n, Mp), mean_q, var_q (Mp), Xq (Mp, D), and
// cov_s (n + p + q, Mp) in the place of cov_g, one column per point: P_jk = cov_s[n + p + k][col(b, j)] / s^2 + os k_t(x_j, x_k).
// Nothing of the gradient is formed or read (mu_g, var_g, Xt and grad are NULL), and U / SL leave the LDS.
#pragma once
#include "gp_studies_formulas.h"   // SA_DEV / SA_SYNC, sa_kernel_and_slope, the acquisition codes
#include "gp_qacqf_columns.h"

namespace scaml {

constexpr int QACQF_MAX_Q = 8;           // points per batch
constexpr int QACQF_MAX_SAMPLES = 512;   // base samples
constexpr int QACQF_MAX_ROWS = 96;       // n + q: the GRAD pass's covariance block
constexpr int QACQF_MAX_D = 15;          // (its 16 columns per query point)
constexpr int QACQF_THREADS = 256;
constexpr int QA_CHUNKS = 4;             // the sample axis is summed in four consecutive chunks, met as (c0 + c1) + (c2 + c3)
constexpr int QA_ENTRIES = 73;           // Cbar [8][8] | mubar [8] | value

// qEI and qUCB only: a joint LogEI is not defined here
SA_DEV bool qa_acqf_valid(int acqf) { return acqf == SA_ACQF_UCB || acqf == SA_ACQF_EI; }

struct QAcqfParams {
  const double* Knq;            // (n, Mq)
  const double* Z;              // (n, Mq) Knn^-1 Knq
  const double* alpha;          // (n)
  const double* mean_q;         // (Mq)
  const double* var_q;          // (Mq)
  double m_all, s_all;
  const int32_t* info;          // (1) or NULL: != 0, every output is NaN
  const double* cov_g;          // (n + q, Mq * 16) weighted sums of (5g)
  const double* mu_g;           // (Mq * 16)
  const double* var_g;          // (Mq * 16)
  const double* Xt;             // (n, D)
  const double* Xq;             // (Mq, D)
  const double* theta;          // (D + 2) target kernel
  const double* base_samples;   // (S, q)
  double acqf_param;            // qEI: best_f; qUCB: beta
  double* value;                // (B)
  double* grad;                 // (Mq, D) or NULL
  double* jitter_used;          // (B) or NULL
  int32_t* info_out;            // (B) or NULL
  int n, Mq, q, S, D, kind, acqf, pad_;
};

// (7q): the pending set, shared by all batches.  In QAcqfParams then: cov_g (n + p + q, Mq * 16), base_samples (S, q + p).
struct QAcqfPending {
  const double* Xp;         // (p, D)
  const double* Zp;         // (n, p) Knn^-1 Knp
  const double* mu_p;       // (p)    target posterior mean of the pending points, original units
  const double* Sigma_pp;   // (p, p) ... and their covariance among themselves, no observation noise
  int p, pad_;
};
struct QAcqfPendingParams {
  QAcqfParams a;
  QAcqfPending pe;
};

// ---- LDS of the tail, in doubles (8 x 8 matrices with row stride 8, whatever q) -----------------------------------------------------
//   Sigma | mu [8] | C | C^-1 | Cbar, then Phi C^-1 | mubar [8] | Phi, then C^-T Phi C^-1 | Sigmabar | out [8] | part [4][80] |
//   eps [S][q] | a, wm, wc, j* [4][S]
constexpr int QA_SG = 0, QA_MU = 64, QA_C = 72, QA_CI = 136, QA_CB = 200, QA_MB = 264, QA_T1 = 272, QA_SB = 336, QA_OUT = 400, QA_PART = 408,
              QA_EPS = QA_PART + QA_CHUNKS * 80;
constexpr int QA_OUT_VALUE = 0, QA_OUT_JITTER = 1, QA_OUT_INFO = 2;
constexpr size_t qa_tail_lds_doubles(int q, int S) { return (size_t)QA_EPS + (size_t)S * (size_t)(q + 4); }
// ... and of a whole batch: the tail, then  Knq [n][8] | Z [n][8] | U, SL [2][8][n + q] | bad [8]
constexpr size_t qa_lds_doubles(int n, int q, int S) { return qa_tail_lds_doubles(q, S) + 16 * (size_t)n + 16 * (size_t)(n + q) + 8; }
// ... and with p pending points: the tail at q + p, Knq | Z as above, U, SL [2][8][n + p + q] | bad [8] | Zp [n][8]
constexpr size_t qa_pending_lds_doubles(int n, int q, int p, int S) {
  return qa_tail_lds_doubles(q + p, S) + 16 * (size_t)n + 16 * (size_t)(n + p + q) + 8 + 8 * (size_t)n;
}
// ... and of the value-only batch (7r): the tail at q + p, Knq | Z as above, bad [8] | Zp [n][8] -- no U, SL
constexpr size_t qa_value_lds_doubles(int n, int q, int p, int S) { return qa_tail_lds_doubles(q + p, S) + 16 * (size_t)n + 8 + 8 * (size_t)n; }

// Everything from "Sigma, mu given" onwards, by `nthr` cooperating threads: t[QA_SG] (both triangles; only the lower one is read) and
// t[QA_MU] hold the joint posterior of the q points, entries past q are zero.  Leaves value, jitter and info in t[QA_OUT], mubar in
// t[QA_MB] and Sigmabar (symmetric: d value = sum_jk Sigmabar_jk dSigma_jk) in t[QA_SB].  info == 1: no jitter of the ladder made
// Sigma positive definite (or it holds a NaN); value, mubar and Sigmabar are NaN then.
SA_DEV void qa_tail(double* t, int q, int S, int acqf, double par, const double* __restrict__ base_samples, int tid, int nthr) {
  double* Sg = t + QA_SG;
  double* mu = t + QA_MU;
  double* C = t + QA_C;
  double* Ci = t + QA_CI;
  double* Cb = t + QA_CB;
  double* mb = t + QA_MB;
  double* T1 = t + QA_T1;
  double* Sb = t + QA_SB;
  double* out = t + QA_OUT;
  double* part = t + QA_PART;
  double* eps = t + QA_EPS;
  double* as = eps + (size_t)S * q;
  double* wm = as + S;
  double* wc = wm + S;
  double* js = wc + S;
  const double nan = NAN;

  for (int e = tid; e < S * q; e += nthr) eps[e] = base_samples[e];

  // ---- the jitter ladder: right-looking Cholesky of the lower triangle, a column per step; every thread reads the same pivots, so
  // `ok` and the attempt count are uniform over the workgroup
  bool ok = false;
  double jit = 0.0;
  for (int att = 0; att < 4 && !ok; ++att) {
    jit = att == 0 ? 0.0 : (att == 1 ? 1e-8 : (att == 2 ? 1e-7 : 1e-6));
    SA_SYNC();
    for (int e = tid; e < 64; e += nthr) {
      const int i = e >> 3, j = e & 7;
      C[e] = (i < q && j <= i) ? Sg[e] + (i == j ? jit : 0.0) : 0.0;
    }
    SA_SYNC();
    ok = true;
    for (int k = 0; k < q; ++k) {
      const double piv = C[k * 8 + k];
      ok = ok && piv > 0.0 && piv <= 1.7976931348623157e308;   // (a NaN fails both)
      const double d = sqrt(piv);
      SA_SYNC();
      for (int i = k + tid; i < q; i += nthr) C[i * 8 + k] = i == k ? d : C[i * 8 + k] / d;
      SA_SYNC();
      for (int e = tid; e < 64; e += nthr) {
        const int i = e >> 3, j = e & 7;
        if (i < q && j > k && j <= i) C[e] = fma(-C[i * 8 + k], C[j * 8 + k], C[e]);
      }
      SA_SYNC();
    }
  }
  if (!ok) {
    for (int e = tid; e < 64; e += nthr) Sb[e] = nan;
    for (int e = tid; e < 8; e += nthr) mb[e] = nan;
    if (tid == 0) {
      out[QA_OUT_VALUE] = nan;
      out[QA_OUT_JITTER] = nan;
      out[QA_OUT_INFO] = 1.0;
    }
    SA_SYNC();
    return;
  }

  // ---- C^-1, a column per thread by forward substitution (rows ascending)
  for (int c = tid; c < 8; c += nthr) {
    for (int i = 0; i < 8; ++i) {
      double x = 0.0;
      if (c < q && i < q && i >= c) {
        double acc = i == c ? 1.0 : 0.0;
        for (int k = c; k < i; ++k) acc = fma(-C[i * 8 + k], Ci[k * 8 + c], acc);
        x = acc / C[i * 8 + i];
      }
      Ci[i * 8 + c] = x;
    }
  }
  SA_SYNC();

  // ---- the samples: f = mu + C eps; the utility, its arg-max and what it adds to mubar (wm) and to row j* of Cbar (wc eps)
  const double ucb_c = sqrt(par * 1.5707963267948966192);   // sqrt(beta pi / 2)
  for (int s = tid; s < S; s += nthr) {
    double ev[8], z[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) ev[k] = k < q ? eps[(size_t)s * q + k] : 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k <= j; ++k) acc = fma(C[j * 8 + k], ev[k], acc);   // (rows past q are zero)
      z[j] = acc;
    }
    double best = -INFINITY, zb = 0.0, nanp = 0.0;
    int jb = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double g = acqf == SA_ACQF_EI ? par - (mu[j] + z[j]) : ucb_c * fabs(z[j]) - mu[j];
      if (j < q) {
        nanp += g - g;   // (a NaN or infinite utility loses every comparison: this puts it back into the value)
        if (g > best) {
          best = g;
          jb = j;
          zb = z[j];
        }
      }
    }
    double a, m, c;
    if (acqf == SA_ACQF_EI) {
      const bool on = best > 0.0;
      a = on ? best : 0.0;
      m = c = on ? -1.0 : 0.0;
    } else {
      a = best;
      m = -1.0;
      c = zb > 0.0 ? ucb_c : (zb < 0.0 ? -ucb_c : 0.0);
    }
    as[s] = a + nanp;
    wm[s] = m;
    wc[s] = c;
    js[s] = (double)jb;
  }
  SA_SYNC();

  // ---- sums over the samples: one thread per (chunk, entry), the chunk's samples ascending
  const int chunk = (S + QA_CHUNKS - 1) / QA_CHUNKS;
  for (int w = tid; w < QA_CHUNKS * QA_ENTRIES; w += nthr) {
    const int ch = w / QA_ENTRIES, e = w - ch * QA_ENTRIES;
    const int s_lo = ch * chunk, s_hi = s_lo + chunk < S ? s_lo + chunk : S;
    double acc = 0.0;
    if (e < 64) {
      const int j = e >> 3, k = e & 7;
      if (j < q && k <= j) {
        const double jd = (double)j;
        for (int s = s_lo; s < s_hi; ++s) acc += js[s] == jd ? wc[s] * eps[(size_t)s * q + k] : 0.0;
      }
    } else if (e < 72) {
      const double jd = (double)(e - 64);
      for (int s = s_lo; s < s_hi; ++s) acc += js[s] == jd ? wm[s] : 0.0;
    } else {
      for (int s = s_lo; s < s_hi; ++s) acc += as[s];
    }
    part[ch * 80 + e] = acc;
  }
  SA_SYNC();
  const double invS = 1.0 / (double)S;
  for (int e = tid; e < QA_ENTRIES; e += nthr) {
    const double sum = ((part[e] + part[80 + e]) + (part[160 + e] + part[240 + e])) * invS;
    if (e < 64) Cb[e] = sum;
    else if (e < 72) mb[e - 64] = sum;
    else out[QA_OUT_VALUE] = sum;
  }
  if (tid == 0) {
    out[QA_OUT_JITTER] = jit;
    out[QA_OUT_INFO] = 0.0;
  }
  SA_SYNC();

  // ---- back through the factor: Phi = tril(C^T Cbar), diagonal halved; Sigmabar = sym(C^-T Phi C^-1)
  for (int e = tid; e < 64; e += nthr) {
    const int i = e >> 3, j = e & 7;
    double acc = 0.0;
    if (j <= i)
      for (int k = i; k < 8; ++k) acc = fma(C[k * 8 + i], Cb[k * 8 + j], acc);
    T1[e] = i == j ? 0.5 * acc : acc;
  }
  SA_SYNC();
  for (int e = tid; e < 64; e += nthr) {   // Phi C^-1 (into Cbar's place)
    const int i = e >> 3, j = e & 7;
    double acc = 0.0;
    for (int k = 0; k < 8; ++k) acc = fma(T1[i * 8 + k], Ci[k * 8 + j], acc);
    Cb[e] = acc;
  }
  SA_SYNC();
  for (int e = tid; e < 64; e += nthr) {   // C^-T (Phi C^-1) (into Phi's place)
    const int i = e >> 3, j = e & 7;
    double acc = 0.0;
    for (int k = 0; k < 8; ++k) acc = fma(Ci[k * 8 + i], Cb[k * 8 + j], acc);
    T1[e] = acc;
  }
  SA_SYNC();
  for (int e = tid; e < 64; e += nthr) {
    const int i = e >> 3, j = e & 7;
    Sb[e] = 0.5 * (T1[i * 8 + j] + T1[j * 8 + i]);
  }
  SA_SYNC();
}

// Batch b of the call by `nthr` cooperating threads; `lds`: qa_lds_doubles(n, q, S).  (Every branch up to a barrier is uniform over
// the workgroup.)  PEND: (7q), `pe.p` pending points behind the q moving ones; `lds`: qa_pending_lds_doubles(n, q, p, S).  Without
// PEND `pe` is not read and P below is the constant 0: (7p) as it was, instruction for instruction (a wrapper around the template
// instead of the default argument reorders three instructions of that kernel; tools/dev_isa_diff.py).
// VAL: (7r), the value layout -- p.Mq is Mp, the batch's first column comes from the column map, a point has ONE column of p.cov_g
// (which holds cov_s), `lds`: qa_value_lds_doubles(n, q, p, S), and the body ends with the value.
template <bool PEND = false, bool VAL = false>
SA_DEV void qa_batch(const QAcqfParams& p, double* lds, int b, int tid, int nthr, const QAcqfPending& pe = QAcqfPending{}) {
  constexpr size_t CS = VAL ? 1 : 16;   // columns of the source sums per query point
  const int P = PEND ? pe.p : 0;
  const int n = p.n, q = p.q, S = p.S, D = p.D, Mq = p.Mq, R = n + P + q, Q = q + P;
  const size_t q0 = VAL ? (size_t)qav_column(b, 0, q) : (size_t)b * q, W = (size_t)Mq * CS;
  const double nan = NAN;
  if (p.info && p.info[0] != 0) {   // the target's training block was not positive definite even with jitter
    if (tid == 0) {
      p.value[b] = nan;
      if (p.jitter_used) p.jitter_used[b] = nan;
      if (p.info_out) p.info_out[b] = 1;
    }
    if (p.grad)
      for (int e = tid; e < q * D; e += nthr) p.grad[q0 * D + e] = nan;
    return;
  }
  double* t = lds;
  double* Kq = lds + qa_tail_lds_doubles(Q, S);   // [a][8]
  double* Zq = Kq + (size_t)n * 8;                // [a][8]
  double* U = Zq + (size_t)n * 8;                 // [j][R]: the weight of row a in point j's gradient, / s^2
  double* SL = U + (VAL ? 0 : (size_t)8 * R);     // [j][R]: that weight times 2 os dk_t / d(d2)   (VAL: neither is there)
  double* badp = SL + (VAL ? 0 : (size_t)8 * R);  // [0] the batch's coordinates, [1 .. 7] shares of the pending set's arrays
  double* Zpl = badp + 8;                         // [a][8] (PEND)
  const double s = p.s_all, s2 = s * s, inv_s2 = 1.0 / s2;
  const double os = p.theta[D];

  for (int e = tid; e < n * q; e += nthr) {
    const int a = e / q, j = e - a * q;
    Kq[a * 8 + j] = p.Knq[(size_t)a * Mq + q0 + j];
    Zq[a * 8 + j] = p.Z[(size_t)a * Mq + q0 + j];
  }
  if constexpr (PEND)
    for (int e = tid; e < n * P; e += nthr) Zpl[(e / P) * 8 + e % P] = pe.Zp[e];
  SA_SYNC();
  // ---- the joint posterior of the batch: one thread per entry of Sigma (lower triangle, mirrored) and of mu, training points ascending
  for (int e = tid; e < QA_ENTRIES + (PEND ? 7 : 0); e += nthr) {
    if (e < 64) {
      const int j = e >> 3, k = e & 7;
      if (j >= Q || k >= Q) {
        t[QA_SG + e] = 0.0;
      } else if (PEND && k <= j && j >= q) {
        // a pending row: against a moving point k the mixed block (the pending point is the ANCHOR of strip k: row n + jp of cov_g),
        // against a pending one the given Sigma_pp
        const int jp = j - q;
        double v;
        if (k >= q) {
          v = pe.Sigma_pp[jp * P + (k - q)];
        } else {
          double kz = 0.0;
          for (int a = 0; a < n; ++a) kz = fma(Kq[a * 8 + k], Zpl[a * 8 + jp], kz);
          double d2 = 0.0;
          for (int d = 0; d < D; ++d) {
            const double df = (p.Xq[(q0 + k) * D + d] - pe.Xp[jp * D + d]) / p.theta[d];
            d2 = fma(df, df, d2);
          }
          double k0, dk;
          sa_kernel_and_slope(p.kind, d2, os, k0, dk);
          v = s2 * (p.cov_g[(size_t)(n + jp) * W + (q0 + k) * CS] * inv_s2 + k0 + (d2 - d2) - kz);
        }
        t[QA_SG + j * 8 + k] = v;
        t[QA_SG + k * 8 + j] = v;
      } else if (k <= j) {
        double kz = 0.0;
        for (int a = 0; a < n; ++a) kz = fma(Kq[a * 8 + j], Zq[a * 8 + k], kz);
        double prior;
        if (j == k) {
          prior = p.var_q[q0 + j];
        } else {
          double d2 = 0.0;
          for (int d = 0; d < D; ++d) {
            const double df = (p.Xq[(q0 + j) * D + d] - p.Xq[(q0 + k) * D + d]) / p.theta[d];
            d2 = fma(df, df, d2);
          }
          double k0, dk;
          sa_kernel_and_slope(p.kind, d2, os, k0, dk);
          prior = p.cov_g[(size_t)(n + P + k) * W + (q0 + j) * CS] * inv_s2 + k0 + (d2 - d2);
        }
        const double v = s2 * (prior - kz);
        t[QA_SG + j * 8 + k] = v;
        t[QA_SG + k * 8 + j] = v;
      }
    } else if (e < 72) {
      const int j = e - 64;
      double m = 0.0;
      if (j < q) {
        double acc = p.mean_q[q0 + j];
        for (int a = 0; a < n; ++a) acc = fma(Kq[a * 8 + j], p.alpha[a], acc);
        m = fma(s, acc, p.m_all);
      }
      if (PEND && j >= q && j < Q) m = pe.mu_p[j - q];
      t[QA_MU + j] = m;
    } else if (!PEND || e == 72) {
      // a NaN / infinite coordinate anywhere in the batch: sum (x - x) is 0, or NaN then
      double bad = 0.0;
      for (int i = 0; i < q * D; ++i) {
        const double x = p.Xq[q0 * D + i];
        bad += x - x;
      }
      badp[0] = bad;
    } else if constexpr (PEND) {
      // ... or anywhere in the pending set's arrays, which every batch shares: seven threads, every seventh element each
      const int w = e - QA_ENTRIES, nx = P * D, nz = nx + n * P, nm = nz + P, ns = nm + P * P;
      double bad = 0.0;
      for (int i = w; i < ns; i += 7) {
        const double x = i < nx ? pe.Xp[i] : (i < nz ? pe.Zp[i - nx] : (i < nm ? pe.mu_p[i - nz] : pe.Sigma_pp[i - nm]));
        bad += x - x;
      }
      badp[1 + w] = bad;
    }
  }
  SA_SYNC();
  qa_tail(t, Q, S, p.acqf, p.acqf_param, p.base_samples, tid, nthr);

  const bool failed = t[QA_OUT + QA_OUT_INFO] != 0.0;
  double value = failed ? nan : t[QA_OUT + QA_OUT_VALUE] + badp[0];
  if constexpr (PEND)
    for (int w = 1; w < 8; ++w) value += badp[w];   // (zeros, or NaN)
  if (tid == 0) {
    p.value[b] = value;
    if (p.jitter_used) p.jitter_used[b] = t[QA_OUT + QA_OUT_JITTER];
    if (p.info_out) p.info_out[b] = failed ? 1 : 0;
  }
  if (VAL || !p.grad) return;
  if (value != value) {   // (NaN: uniform over the workgroup, all of them read the same value)
    for (int e = tid; e < q * D; e += nthr) p.grad[q0 * D + e] = nan;
    return;
  }
  // ---- the gradient.  Row a of point j: a training point (weight mbar_j alpha_a - 2 sum_k Sbar_jk Z[a][k]) or batch mate k = a - n
  // (weight 2 Sbar_jk, nothing for the point itself: its row is in dvar_q); the slope of the target kernel once per (j, a) for all D
  const double* mb = t + QA_MB;
  const double* Sb = t + QA_SB;
  for (int e = tid; e < q * R; e += nthr) {
    const int j = e / R, a = e - j * R;
    double u;
    const double* xa;
    if (a < n) {
      double sz = 0.0;
      for (int k = 0; k < q; ++k) sz = fma(Sb[j * 8 + k], Zq[a * 8 + k], sz);
      if constexpr (PEND)
        for (int k = 0; k < P; ++k) sz = fma(Sb[j * 8 + q + k], Zpl[a * 8 + k], sz);
      u = s * mb[j] * p.alpha[a] - 2.0 * s2 * sz;
      xa = p.Xt + (size_t)a * D;
    } else if (PEND && a < n + P) {   // a pending point: held fixed, so only this side of the pair
      const int k = a - n;
      u = 2.0 * s2 * Sb[j * 8 + q + k];
      xa = pe.Xp + (size_t)k * D;
    } else {
      const int k = a - n - P;
      u = k == j ? 0.0 : 2.0 * s2 * Sb[j * 8 + k];
      xa = p.Xq + (q0 + k) * D;
    }
    const double* xj = p.Xq + (q0 + j) * D;
    double d2 = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = (xj[d] - xa[d]) / p.theta[d];
      d2 = fma(df, df, d2);
    }
    double k0, dk;
    sa_kernel_and_slope(p.kind, d2, os, k0, dk);
    U[j * R + a] = u * inv_s2;
    SL[j * R + a] = 2.0 * u * dk;
  }
  SA_SYNC();
  double* gl = t + QA_PART;   // [q][D], at most 120 doubles: the chunk sums are spent
  for (int e = tid; e < q * D; e += nthr) {
    const int j = e / D, d = e - j * D;
    const size_t col = (q0 + j) * 16 + 1 + d;
    const double il2 = 1.0 / (p.theta[d] * p.theta[d]);
    const double xjd = p.Xq[(q0 + j) * D + d];
    double acc = fma(mb[j], p.mu_g[col], Sb[j * 8 + j] * p.var_g[col]);
    for (int a = 0; a < R; ++a) {
      double xad;
      if (PEND && a >= n && a < n + P) xad = pe.Xp[(size_t)(a - n) * D + d];
      else xad = a < n ? p.Xt[(size_t)a * D + d] : p.Xq[(q0 + a - n - P) * D + d];
      acc = fma(U[j * R + a], p.cov_g[(size_t)a * W + col], acc);
      acc = fma(SL[j * R + a], (xjd - xad) * il2, acc);
    }
    gl[e] = acc;
  }
  SA_SYNC();
  // a NaN in ONE derivative column of mu_g / var_g / cov_g reaches one entry only, next to a finite value: every entry of that point's
  // gradient is NaN where the results are stored, the rule of (7f) (a select: finite inputs stay bit for bit what they were)
  for (int e = tid; e < q * D; e += nthr) {
    const int j = e / D;
    bool bad = false;
    for (int d = 0; d < D; ++d) bad = bad || gl[j * D + d] != gl[j * D + d];
    p.grad[q0 * D + e] = bad ? nan : gl[e];
  }
}

// (7q)
SA_DEV void qa_batch_pending(const QAcqfPendingParams& pp, double* lds, int b, int tid, int nthr) {
  qa_batch<true>(pp.a, lds, b, tid, nthr, pp.pe);
}

// (7r): value only, from the value layout, p >= 0 pending points
SA_DEV void qa_batch_value(const QAcqfPendingParams& pp, double* lds, int b, int tid, int nthr) {
  qa_batch<true, true>(pp.a, lds, b, tid, nthr, pp.pe);
}

}  // namespace scaml
