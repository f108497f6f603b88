// The five-point essential-matrix solver of sfmloc_relative_poses (include/sfmloc.h "Relative poses", the paragraph
// "five-point solver"), and the decomposition of an essential matrix into its four (R, t).  tests/relpose_np.py restates
// every operation; only + - * / sqrt in f64, unfused (-ffp-contract=off), every sum in a stated order, every loop with a
// fixed trip count.
//
// One hypothesis is solved by a group of kRpGroup = 16 lanes of one wave (four groups per wave), its matrices in LDS
// (RpGroupLds): the 9 x 9 G and V of the Jacobi null space and the 10 x 20 constraint matrix are 362 doubles, 724 VGPRs
// in one lane.  Lane k of the group owns row k of each rotation's update (nine lanes busy), row k of the Gauss-Jordan
// elimination (ten) and the k-th real root of the tenth-degree polynomial (ten); what every lane needs (a rotation's c
// and s, a pivot, the polynomial) every lane computes itself from the same LDS entries, the same bits.  The phases are
// separated by wave-level LDS fences: the four groups of a wave run the same instruction stream, no trip count depends
// on the data.  Which lane computes a value never changes it, so the code below also runs on the host, one lane after
// the other per phase (RP_LANES): tests/cpp/essential_host.cpp is that instantiation, compared bit for bit with the
// restatement on a machine without a GPU (tests/test_relpose_cpu.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RP_HD __host__ __device__ inline
#else
#define RP_HD inline
#endif

namespace sfmloc {
namespace essential {

constexpr int kRpGroup = 16;            // lanes per hypothesis
constexpr int kRpSweeps = 10;           // geom_device.h kJacobiSweeps
constexpr int kRpMaxModels = 10;
constexpr double kRpRankTol = 1e-12;    // no model when the fifth smallest eigenvalue of G <= this * the largest
constexpr double kRpPivotFloor = 1e-13; // no model when a Gauss-Jordan pivot is not larger in magnitude
constexpr int kRpBisect = 48;           // bisection steps per root over the Cauchy bound
constexpr int kRpNewton = 3;            // Newton steps after them, each kept only inside the last bracket
constexpr int kRpPolish = 2;            // Newton steps on the determinant of the polynomial matrix itself

struct RpGroupLds {
  double GV[162];  // G [9][9], V [9][9]; then the Sturm chain [11][11] and the derivative [10] at 121
  double N[36];    // X, Y, Z, W: the null space, [4][9]
  double M[200];   // the design matrix [5][9], then the constraints [10][20]
  double Eo[90];   // the models per root, before they are packed
  int flag[kRpMaxModels];
  int pad[2];
};

#if defined(__HIP_DEVICE_COMPILE__)
#define RP_LANES(l) for (int l = (int)(threadIdx.x & (kRpGroup - 1)), rp_once = 1; rp_once; rp_once = 0)
#define RP_SYNC()                                           \
  do {                                                      \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
    __builtin_amdgcn_wave_barrier();                        \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
  } while (0)
#else
#define RP_LANES(l) for (int l = 0; l < kRpGroup; ++l)
#define RP_SYNC() do {} while (0)
#endif

RP_HD double rp_abs(double x) { return x < 0.0 ? -x : x; }
RP_HD bool rp_finite(double x) { return x - x == 0.0; }  // (inf - inf and NaN - NaN are NaN)

// q += a b for two linear forms in (x, y, z, 1); quadratic monomials x^2 xy xz x y^2 yz y z^2 z 1; terms in the order p, r
RP_HD void rp_mul11(double (&q)[10], const double (&a)[4], const double (&b)[4]) {
  constexpr int I2[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) q[I2[p][r]] = q[I2[p][r]] + a[p] * b[r];
}
// c += q a; cubic monomials x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1; terms in the order m, p
RP_HD void rp_mul21(double (&c)[20], const double (&q)[10], const double (&a)[4]) {
  constexpr int I3[10][4] = {{0, 2, 4, 5},   {2, 3, 8, 9},     {4, 8, 10, 11},   {5, 9, 11, 12},   {3, 1, 6, 7},
                             {8, 6, 13, 14}, {9, 7, 14, 15}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
#pragma unroll
  for (int m = 0; m < 10; ++m)
#pragma unroll
    for (int p = 0; p < 4; ++p) c[I3[m][p]] = c[I3[m][p]] + q[m] * a[p];
}
RP_HD void rp_lin(const double *N, int e, double (&a)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t) a[t] = N[9 * t + e];
}
template <int K>
RP_HD void rp_zero(double (&q)[K]) {
#pragma unroll
  for (int i = 0; i < K; ++i) q[i] = 0.0;
}
// q = E_a E_b - E_c E_d (entries of the linear-form matrix)
RP_HD void rp_minor(const double *N, int a, int b, int c, int d, double (&q)[10]) {
  double l0[4], l1[4], q2[10];
  rp_zero(q);
  rp_zero(q2);
  rp_lin(N, a, l0);
  rp_lin(N, b, l1);
  rp_mul11(q, l0, l1);
  rp_lin(N, c, l0);
  rp_lin(N, d, l1);
  rp_mul11(q2, l0, l1);
#pragma unroll
  for (int i = 0; i < 10; ++i) q[i] = q[i] - q2[i];
}
// q = (E E^T)_ij = sum over k of E_ik E_jk, k ascending
RP_HD void rp_eet(const double *N, int i, int j, double (&q)[10]) {
  rp_zero(q);
#pragma unroll 1
  for (int k = 0; k < 3; ++k) {
    double l0[4], l1[4];
    rp_lin(N, 3 * i + k, l0);
    rp_lin(N, 3 * j + k, l1);
    rp_mul11(q, l0, l1);
  }
}
// row r of the constraint matrix: 0 det E; 1 + 3 i + j the (i, j) entry of (E E^T - tr(E E^T) / 2) E
RP_HD void rp_constraint_row(const double *N, int r, double *out) {
  double c[20];
  if (r == 0) {
    double q[10], l[4], c2[20], c3[20];
    rp_zero(c);
    rp_zero(c2);
    rp_zero(c3);
    rp_minor(N, 4, 8, 5, 7, q);
    rp_lin(N, 0, l);
    rp_mul21(c, q, l);
    rp_minor(N, 3, 8, 5, 6, q);
    rp_lin(N, 1, l);
    rp_mul21(c2, q, l);
    rp_minor(N, 3, 7, 4, 6, q);
    rp_lin(N, 2, l);
    rp_mul21(c3, q, l);
#pragma unroll
    for (int i = 0; i < 20; ++i) c[i] = (c[i] - c2[i]) + c3[i];
  } else {
    const int i = (r - 1) / 3, j = (r - 1) % 3;
    double half[10], q[10], l[4];
    rp_eet(N, 0, 0, half);
    rp_eet(N, 1, 1, q);
#pragma unroll
    for (int t = 0; t < 10; ++t) half[t] = half[t] + q[t];
    rp_eet(N, 2, 2, q);
#pragma unroll
    for (int t = 0; t < 10; ++t) half[t] = 0.5 * (half[t] + q[t]);
    rp_zero(c);
#pragma unroll 1
    for (int k = 0; k < 3; ++k) {
      rp_eet(N, i, k, q);
      if (i == k) {
#pragma unroll
        for (int t = 0; t < 10; ++t) q[t] = q[t] - half[t];
      }
      rp_lin(N, 3 * k + j, l);
      rp_mul21(c, q, l);
    }
  }
#pragma unroll
  for (int i = 0; i < 20; ++i) out[i] = c[i];
}

// rows a (leading x^2 z, y^2 z or xyz) and b (x^2, y^2, xy) of the reduced matrix -> a - z b as polynomials in z
// (coefficient i = z^i): the x part, the y part, the constant part
RP_HD void rp_brow(const double *M, int a, int b, double (&px)[4], double (&py)[4], double (&p1)[5]) {
  const double *ea = M + 20 * a, *eb = M + 20 * b;
  px[0] = ea[12];
  px[1] = ea[11] - eb[12];
  px[2] = ea[10] - eb[11];
  px[3] = -eb[10];
  py[0] = ea[15];
  py[1] = ea[14] - eb[15];
  py[2] = ea[13] - eb[14];
  py[3] = -eb[13];
  p1[0] = ea[19];
  p1[1] = ea[18] - eb[19];
  p1[2] = ea[17] - eb[18];
  p1[3] = ea[16] - eb[17];
  p1[4] = -eb[16];
}
// c = a b, terms added in the order i, j from 0.0
template <int NA, int NB>
RP_HD void rp_pm(const double (&a)[NA], const double (&b)[NB], double (&c)[NA + NB - 1]) {
  rp_zero(c);
#pragma unroll
  for (int i = 0; i < NA; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) c[i + j] = c[i + j] + a[i] * b[j];
}
template <int NA, int NB>
RP_HD void rp_pm_diff(const double (&a)[NA], const double (&b)[NB], const double (&c)[NB], const double (&d)[NA],
                      double (&out)[NA + NB - 1]) {  // a b - c d
  double t[NA + NB - 1];
  rp_pm(a, b, out);
  rp_pm(c, d, t);
#pragma unroll
  for (int i = 0; i < NA + NB - 1; ++i) out[i] = out[i] - t[i];
}
RP_HD double rp_horner(const double *p, int deg, double x) {
  double v = p[deg];
  for (int i = deg - 1; i >= 0; --i) v = v * x + p[i];
  return v;
}
template <int DEG>
RP_HD double rp_horner_s(const double (&p)[DEG + 1], double x) {
  double v = p[DEG];
#pragma unroll
  for (int i = DEG - 1; i >= 0; --i) v = v * x + p[i];
  return v;
}
RP_HD double rp_det3(const double (&a)[3], const double (&b)[3], const double (&c)[3]) {
  return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}
// sign changes of the Sturm chain (member i: degree 10 - i, at chain + 11 i) at x; zeros and NaN are skipped
RP_HD int rp_sign_changes(const double *chain, double x) {
  int cnt = 0, last = 0;
#pragma unroll 1
  for (int i = 0; i < 11; ++i) {
    const double v = rp_horner(chain + 11 * i, 10 - i, x);
    const int s = v > 0.0 ? 1 : (v < 0.0 ? -1 : 0);
    cnt += (s != 0 && last != 0 && s != last) ? 1 : 0;
    last = s != 0 ? s : last;
  }
  return cnt;
}

// The solver.  x1, x2: the five bearing pairs (x, y interleaved), the same values in every lane of the group.  Returns
// the number of models (the same in every lane) and packs them, unit Frobenius norm, ascending root z, into dst [<= 10][9]
// (the group's own, LDS or global).  Executed by whole waves; a group without a hypothesis runs on zeros.
RP_HD int five_point_group(RpGroupLds &L, const double *x1, const double *x2, double *dst) {
  double *const G = L.GV, *const V = L.GV + 81, *const chain = L.GV, *const dp = L.GV + 121;
  // design matrix (row r: the pair r) and G = D^T D, rows added in order
  RP_LANES(l) {
    for (int r = l; r < 5; r += kRpGroup) {
      const double a = x1[2 * r], b = x1[2 * r + 1], u = x2[2 * r], v = x2[2 * r + 1];
      double *d = L.M + 9 * r;
      d[0] = u * a;
      d[1] = u * b;
      d[2] = u;
      d[3] = v * a;
      d[4] = v * b;
      d[5] = v;
      d[6] = a;
      d[7] = b;
      d[8] = 1.0;
    }
  }
  RP_SYNC();
  RP_LANES(l) {
    for (int i = l; i < 9; i += kRpGroup)
      for (int j = 0; j < 9; ++j) {
        double acc = L.M[i] * L.M[j];
        for (int r = 1; r < 5; ++r) acc = acc + L.M[9 * r + i] * L.M[9 * r + j];
        G[9 * i + j] = acc;
        V[9 * i + j] = i == j ? 1.0 : 0.0;
      }
  }
  RP_SYNC();
  // geom_device.h jacobi_fixed<9>
#pragma unroll 1
  for (int sw = 0; sw < kRpSweeps; ++sw)
#pragma unroll 1
    for (int p = 0; p < 8; ++p)
#pragma unroll 1
      for (int q = p + 1; q < 9; ++q) {
        const double apq = G[9 * p + q];
        const bool skip = apq == 0.0;
        const double theta = (G[9 * q + q] - G[9 * p + p]) / (2.0 * apq);
        const double ath = theta < 0.0 ? -theta : theta;
        const double t = (theta < 0.0 ? -1.0 : 1.0) / (ath + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0);
        const double s = t * c;
        RP_SYNC();  // every lane has read the three entries
        RP_LANES(l) {
          for (int k = l; k < 9; k += kRpGroup) {  // G J: columns p and q
            const double akp = G[9 * k + p], akq = G[9 * k + q];
            const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
            G[9 * k + p] = skip ? akp : np_;
            G[9 * k + q] = skip ? akq : nq_;
          }
        }
        RP_SYNC();
        RP_LANES(l) {
          for (int k = l; k < 9; k += kRpGroup) {  // J^T (G J): rows p and q
            const double apk = G[9 * p + k], aqk = G[9 * q + k];
            const double np_ = c * apk - s * aqk, nq_ = s * apk + c * aqk;
            G[9 * p + k] = skip ? apk : np_;
            G[9 * q + k] = skip ? aqk : nq_;
          }
        }
        RP_SYNC();
        RP_LANES(l) {
          if (l == 0 && !skip) {
            G[9 * p + q] = 0.0;
            G[9 * q + p] = 0.0;
          }
          for (int k = l; k < 9; k += kRpGroup) {
            const double vkp = V[9 * k + p], vkq = V[9 * k + q];
            const double np_ = c * vkp - s * vkq, nq_ = s * vkp + c * vkq;
            V[9 * k + p] = skip ? vkp : np_;
            V[9 * k + q] = skip ? vkq : nq_;
          }
        }
        RP_SYNC();
      }
  // X, Y, Z, W: the columns of the four smallest diagonal entries, ascending, the first on ties; the fifth for the rank
  int sel[4] = {0, 0, 0, 0};
  double dsel = 0.0;
  {
    unsigned taken = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      double best = 0.0;
      int ib = -1;
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        const double d = G[10 * i];
        const bool take = !((taken >> i) & 1u) && (ib < 0 || d < best);
        best = take ? d : best;
        ib = take ? i : ib;
      }
      taken |= 1u << ib;
      if (t < 4) sel[t] = ib;
      else dsel = best;
    }
  }
  double dmax = G[0];
#pragma unroll
  for (int i = 1; i < 9; ++i) dmax = G[10 * i] > dmax ? G[10 * i] : dmax;
  bool ok = dsel > kRpRankTol * dmax;
  RP_LANES(l) {
    for (int c = l; c < 9; c += kRpGroup)
#pragma unroll
      for (int t = 0; t < 4; ++t) L.N[9 * t + c] = V[9 * c + sel[t]];
  }
  RP_SYNC();
  RP_LANES(l) {
    if (l < 10) rp_constraint_row(L.N, l, L.M + 20 * l);
  }
  RP_SYNC();
  // Gauss-Jordan on the first ten columns, partial pivoting: the largest magnitude, the first on ties
#pragma unroll 1
  for (int c = 0; c < 10; ++c) {
    int pr = c;
    double pa = rp_abs(L.M[20 * c + c]);
    for (int r = c + 1; r < 10; ++r) {
      const double av = rp_abs(L.M[20 * r + c]);
      const bool take = av > pa;
      pa = take ? av : pa;
      pr = take ? r : pr;
    }
    ok = ok && pa > kRpPivotFloor;
    RP_SYNC();
    RP_LANES(l) {
      for (int j = l; j < 20; j += kRpGroup) {
        const double a = L.M[20 * c + j], b = L.M[20 * pr + j];
        L.M[20 * pr + j] = a;
        L.M[20 * c + j] = b;
      }
    }
    RP_SYNC();
    const double piv = L.M[20 * c + c];
    RP_SYNC();
    RP_LANES(l) {
      for (int j = l; j < 20; j += kRpGroup) L.M[20 * c + j] = L.M[20 * c + j] / piv;
    }
    RP_SYNC();
    RP_LANES(l) {
      if (l < 10 && l != c) {
        const double f = L.M[20 * l + c];
        for (int j = 0; j < 20; ++j) L.M[20 * l + j] = L.M[20 * l + j] - f * L.M[20 * c + j];
      }
    }
    RP_SYNC();
  }
  // the 3 x 3 polynomial matrix in z and its determinant
  double p[11];
  {
    double kx[4], ky[4], k1[5], lx[4], ly[4], l1[5], mx[4], my[4], m1[5];
    rp_brow(L.M, 4, 5, kx, ky, k1);
    rp_brow(L.M, 6, 7, lx, ly, l1);
    rp_brow(L.M, 8, 9, mx, my, m1);
    double t1[8], t2[8], t3[7], d1[11], d2[11], d3[11];
    rp_pm_diff(ly, m1, l1, my, t1);  // ly m1 - l1 my
    rp_pm_diff(lx, m1, l1, mx, t2);  // lx m1 - l1 mx
    {
      double u[7];
      rp_pm(lx, my, t3);
      rp_pm(ly, mx, u);
#pragma unroll
      for (int i = 0; i < 7; ++i) t3[i] = t3[i] - u[i];
    }
    rp_pm(kx, t1, d1);
    rp_pm(ky, t2, d2);
    rp_pm(k1, t3, d3);
#pragma unroll
    for (int i = 0; i < 11; ++i) p[i] = (d1[i] - d2[i]) + d3[i];
  }
  // the Sturm chain, every member divided by its largest magnitude (the space of G and V)
  RP_LANES(l) {
    if (l == 0) {
      double mx = rp_abs(p[0]);
#pragma unroll
      for (int i = 1; i < 11; ++i) mx = rp_abs(p[i]) > mx ? rp_abs(p[i]) : mx;
#pragma unroll
      for (int i = 0; i < 11; ++i) chain[i] = p[i] / mx;
      for (int i = 0; i < 10; ++i) dp[i] = (double)(i + 1) * chain[i + 1];
      mx = rp_abs(dp[0]);
      for (int i = 1; i < 10; ++i) mx = rp_abs(dp[i]) > mx ? rp_abs(dp[i]) : mx;
      for (int i = 0; i < 10; ++i) chain[11 + i] = dp[i] / mx;
#pragma unroll 1
      for (int i = 1; i < 10; ++i) {
        const int n = 11 - i;
        const double *a = chain + 11 * (i - 1), *b = chain + 11 * i;
        double *r = chain + 11 * (i + 1);
        const double q1 = a[n] / b[n - 1];
        const double q0 = (a[n - 1] - q1 * b[n - 2]) / b[n - 1];
        for (int j = 0; j < n - 1; ++j) {
          const double a1 = j == 0 ? a[0] : a[j] - q1 * b[j - 1];
          r[j] = -(a1 - q0 * b[j]);
        }
        double m = rp_abs(r[0]);
        for (int j = 1; j < n - 1; ++j) m = rp_abs(r[j]) > m ? rp_abs(r[j]) : m;
        for (int j = 0; j < n - 1; ++j) r[j] = r[j] / m;
      }
    }
  }
  RP_SYNC();
  double bound = rp_abs(chain[0] / chain[10]);
  for (int i = 1; i < 10; ++i) {
    const double a = rp_abs(chain[i] / chain[10]);
    bound = a > bound ? a : bound;
  }
  bound = 1.0 + bound;
  const int vlo = rp_sign_changes(chain, -bound);
  const int nr = vlo - rp_sign_changes(chain, bound);
  RP_LANES(l) {
    if (l < kRpMaxModels) {
      double lo = -bound, hi = bound;
#pragma unroll 1
      for (int it = 0; it < kRpBisect; ++it) {
        const double mid = 0.5 * (lo + hi);
        const bool up = vlo - rp_sign_changes(chain, mid) >= l + 1;
        hi = up ? mid : hi;
        lo = up ? lo : mid;
      }
      double z = 0.5 * (lo + hi);
#pragma unroll 1
      for (int it = 0; it < kRpNewton; ++it) {
        const double zn = z - rp_horner(chain, 10, z) / rp_horner(dp, 9, z);
        z = (zn >= lo && zn <= hi) ? zn : z;
      }
      // two more Newton steps on det B(z) taken from the matrix itself (the expanded coefficients of p have lost digits
      // to cancellation, the matrix has not), each kept when it moves z by at most 1e-6 (1 + |z|)
      double row[3][3];
#pragma unroll 1
      for (int it = 0; it <= kRpPolish; ++it) {
        double drow[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          double px[4], py[4], p1[5];
          rp_brow(L.M, 4 + 2 * r, 5 + 2 * r, px, py, p1);
          row[r][0] = rp_horner_s<3>(px, z);
          row[r][1] = rp_horner_s<3>(py, z);
          row[r][2] = rp_horner_s<4>(p1, z);
          const double dx[3] = {1.0 * px[1], 2.0 * px[2], 3.0 * px[3]};
          const double dy[3] = {1.0 * py[1], 2.0 * py[2], 3.0 * py[3]};
          const double d1[4] = {1.0 * p1[1], 2.0 * p1[2], 3.0 * p1[3], 4.0 * p1[4]};
          drow[r][0] = rp_horner_s<2>(dx, z);
          drow[r][1] = rp_horner_s<2>(dy, z);
          drow[r][2] = rp_horner_s<3>(d1, z);
        }
        if (it == kRpPolish) break;  // (the rows at the final z: x and y below)
        const double f = rp_det3(row[0], row[1], row[2]);
        const double df = (rp_det3(drow[0], row[1], row[2]) + rp_det3(row[0], drow[1], row[2])) + rp_det3(row[0], row[1], drow[2]);
        const double zn = z - f / df;
        z = rp_abs(zn - z) <= 1e-6 * (1.0 + rp_abs(z)) ? zn : z;
      }
      // x and y: the null vector of the polynomial matrix at z, the cross product with the largest third entry
      double n0 = 0.0, n1 = 0.0, n2 = 0.0;
#pragma unroll
      for (int pi = 0; pi < 3; ++pi) {
        const int ra = pi == 2 ? 1 : 0, rb = pi == 0 ? 1 : 2;
        const double c0 = row[ra][1] * row[rb][2] - row[ra][2] * row[rb][1];
        const double c1 = row[ra][2] * row[rb][0] - row[ra][0] * row[rb][2];
        const double c2 = row[ra][0] * row[rb][1] - row[ra][1] * row[rb][0];
        const bool take = pi == 0 || rp_abs(c2) > rp_abs(n2);
        n0 = take ? c0 : n0;
        n1 = take ? c1 : n1;
        n2 = take ? c2 : n2;
      }
      const double x = n0 / n2, y = n1 / n2;
      double E[9], ss = 0.0;
#pragma unroll
      for (int e = 0; e < 9; ++e) {
        E[e] = ((x * L.N[e] + y * L.N[9 + e]) + z * L.N[18 + e]) + L.N[27 + e];
        ss = e == 0 ? E[e] * E[e] : ss + E[e] * E[e];
      }
      const double nrm = sqrt(ss);
      bool fin = true;
#pragma unroll
      for (int e = 0; e < 9; ++e) {
        E[e] = E[e] / nrm;
        fin = fin && rp_finite(E[e]);
        L.Eo[9 * l + e] = E[e];
      }
      L.flag[l] = (ok && l < nr && fin) ? 1 : 0;
    }
  }
  RP_SYNC();
  int nm = 0;
#pragma unroll
  for (int i = 0; i < kRpMaxModels; ++i) nm += L.flag[i];
  RP_LANES(l) {
    if (l < kRpMaxModels && L.flag[l]) {
      int rank = 0;
      for (int i = 0; i < l; ++i) rank += L.flag[i];
      for (int e = 0; e < 9; ++e) dst[9 * rank + e] = L.Eo[9 * l + e];
    }
  }
  RP_SYNC();
  return nm;
}

// sfmloc.h "decomposition": E -> the rotations Ra = U W V^T, Rb = U W^T V^T and the unit translation t = u3; the four
// candidates are (Ra, t), (Ra, -t), (Rb, t), (Rb, -t).  The Jacobi of E^T E is the caller's (geom_device.h
// jacobi_fixed<3>): d its diagonal afterwards, V its eigenvectors in columns.
RP_HD void decompose_from_jacobi(const double *E, const double (&d)[3], const double (&V)[3][3], double *Ra, double *Rb,
                                 double *t) {
  int i1 = 0;
  if (d[1] > d[i1]) i1 = 1;
  if (d[2] > d[i1]) i1 = 2;
  int i2 = -1;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (i != i1 && (i2 < 0 || d[i] > d[i2])) i2 = i;
  const double s1 = sqrt(d[i1]), s2 = sqrt(d[i2]);
  double v1[3], v2[3], u1[3], u2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    v1[i] = V[i][i1];
    v2[i] = V[i][i2];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    u1[i] = ((E[3 * i] * v1[0] + E[3 * i + 1] * v1[1]) + E[3 * i + 2] * v1[2]) / s1;
    u2[i] = ((E[3 * i] * v2[0] + E[3 * i + 1] * v2[1]) + E[3 * i + 2] * v2[2]) / s2;
  }
  const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
  double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
  const double nrm = sqrt((u3[0] * u3[0] + u3[1] * u3[1]) + u3[2] * u3[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) u3[i] = u3[i] / nrm;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Ra[3 * i + j] = (u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3[j];
      Rb[3 * i + j] = (u1[i] * v2[j] - u2[i] * v1[j]) + u3[i] * v3[j];
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = u3[i];
}

}  // namespace essential
}  // namespace sfmloc
