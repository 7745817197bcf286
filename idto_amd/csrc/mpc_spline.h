// mpc_spline.h — the arithmetic of the model-predictive-control shell (include/idto/examples/mpc_controller.h; reference
// examples/mpc_controller.cc:43-138) as pure functions of flat arrays: the not-a-knot cubic fit, its evaluation, the time
// of a guess row, the shift of the nominal trajectory and the row a control knot takes its torques from.  Plain C++, no
// HIP type: the host includes it as it is (PiecewiseCubic, ModelPredictiveController), hipcc compiles the same text for
// the device (`__host__ __device__`, mpc_batch.h), so that a plan fitted or shifted on either side is the same numbers.
// Both sides compile without contraction of a * b + c; the expressions below are evaluated in the order they are written -
// do not regroup them.
//
// A spline of n knots and `dim` components is breaks t[n], values y[knot][dim] and knot derivatives m[knot][dim]; the
// functions work on ONE component, addressed by a pointer to its entry of knot 0 and the stride between knots.
#pragma once

#if defined(__HIPCC__)
#define IDTO_MPC_HD __host__ __device__
#else
#define IDTO_MPC_HD
#endif

namespace idto_spline {

// UpdateInitialGuess (:87-97): the time, relative to the stored plan's start, of row i of the guess
IDTO_MPC_HD inline double guess_time(double start, int i, double time_step) { return start + i * time_step; }

// UpdateAbstractState (:60-69): one entry of the nominal trajectory, moved with the initial condition where selected.
// An entry that is not selected gets (0.0 * difference) added, as the reference adds it.
IDTO_MPC_HD inline double nominal_shift(double q_nom, bool selected, double q0, double q_nom_old0) {
  q_nom += (selected ? 1.0 : 0.0) * (q0 - q_nom_old0);
  return q_nom;
}

// StoreOptimizerSolution (:122-126): control knot i of num_knots takes tau's row min(i, num_knots - 2) - the torques are
// undefined at the last time step, which repeats the row before it
IDTO_MPC_HD inline int control_row(int i, int num_knots) { return i == num_knots - 1 ? i - 1 : i; }

IDTO_MPC_HD inline double spline_slope(const double* t, const double* y, int stride, int i) {
  return (y[(long long)(i + 1) * stride] - y[(long long)i * stride]) / (t[i + 1] - t[i]);
}

// The knot derivatives of one component: m_i from the linear system of C2 continuity
//   h_i m_{i-1} + 2 (h_{i-1} + h_i) m_i + h_{i-1} m_{i+1} = 3 (h_i d_{i-1} + h_{i-1} d_i),  d_i = (y_{i+1} - y_i) / h_i
// closed by the not-a-knot conditions at both ends; two knots: the line, three: the parabola through them.
// The not-a-knot system is TRIDIAGONAL as it stands - row 0 = [h1, h0 + h1], rows i = [h_i, 2 (h_{i-1} + h_i), h_{i-1}],
// row n - 1 = [h_{n-2} + h_{n-3}, h_{n-3}] - and one elimination without pivoting is stable on it: after row 0
// (multiplier 1) row 1's diagonal is h0 + h1 > h0 and the interior rows are diagonally dominant.
// t: n increasing breaks; y, m, w: the component's entries of knot 0 (knot i at [i * stride]); w: n entries of work space
// (the eliminated diagonal; untouched for n < 4).  Returns 0, or 1 for a vanished pivot (m is then not to be used).
IDTO_MPC_HD inline int spline_fit(const double* t, int n, const double* y, double* m, double* w, int stride) {
  const long long st = stride;
  if (n == 2) {   // the line
    m[0] = m[st] = spline_slope(t, y, stride, 0);
    return 0;
  }
  if (n == 3) {   // the parabola through the three points
    const double h0 = t[1] - t[0], h1 = t[2] - t[1];
    const double d0 = spline_slope(t, y, stride, 0), d1 = spline_slope(t, y, stride, 1), a2 = (d1 - d0) / (h0 + h1);
    m[0] = d0 - a2 * h0;
    m[st] = d0 + a2 * h0;
    m[2 * st] = d1 + a2 * h1;
    return 0;
  }
  // the right-hand side goes into m, the diagonal into w
  for (int i = 1; i + 1 < n; ++i) {
    const double hm = t[i] - t[i - 1], hi = t[i + 1] - t[i];
    w[i * st] = 2 * (hm + hi);
    m[i * st] = 3 * (hi * spline_slope(t, y, stride, i - 1) + hm * spline_slope(t, y, stride, i));
  }
  const double h0 = t[1] - t[0], h1 = t[2] - t[1];
  const double hn2 = t[n - 1] - t[n - 2], hn3 = t[n - 2] - t[n - 3];
  const double d = h0 + h1, e = hn2 + hn3;
  w[0] = h1;
  m[0] = ((h0 + 2 * d) * h1 * spline_slope(t, y, stride, 0) + h0 * h0 * spline_slope(t, y, stride, 1)) / d;
  w[(n - 1) * st] = hn3;
  m[(n - 1) * st] = (hn2 * hn2 * spline_slope(t, y, stride, n - 3) + (2 * e + hn2) * hn3 * spline_slope(t, y, stride, n - 2)) / e;
  // lower diagonal: h_i (last row: e); upper diagonal: h_{i-1} (row 0: d)
  for (int i = 1; i < n; ++i) {
    if (w[(i - 1) * st] == 0.0) return 1;
    const double lo = (i == n - 1) ? e : t[i + 1] - t[i];
    const double up = (i == 1) ? d : t[i - 1] - t[i - 2];
    const double f = lo / w[(i - 1) * st];
    w[i * st] -= f * up;
    m[i * st] -= f * m[(i - 1) * st];
  }
  if (w[(n - 1) * st] == 0.0) return 1;
  for (int i = n - 1; i >= 0; --i) {
    const double up = (i == 0) ? d : t[i] - t[i - 1];
    const double s = m[i * st] - (i + 1 < n ? up * m[(i + 1) * st] : 0.0);
    m[i * st] = s / w[i * st];
  }
  return 0;
}

// PiecewisePolynomial::value's choice of the piece: *t clamped to the breaks' range, then the interval by upper_bound
// (a time on a knot belongs to the interval that begins there; the last knot to the last interval)
IDTO_MPC_HD inline int spline_interval(const double* t, int n, double* time) {
  double x = *time;
  x = (x < t[0]) ? t[0] : x;           // std::max(x, front)
  x = (t[n - 1] < x) ? t[n - 1] : x;   // std::min(., back)
  *time = x;
  int lo = 0, hi = n;   // first index whose break is > x
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (x < t[mid]) hi = mid; else lo = mid + 1;
  }
  int i = lo - 1;
  i = (i < 0) ? 0 : i;
  i = (n - 2 < i) ? n - 2 : i;
  return i;
}

// one component of the piece [ti, ti1] at the (clamped) time x
IDTO_MPC_HD inline double spline_piece(double ti, double ti1, double y0, double y1, double m0, double m1, double x) {
  const double h = ti1 - ti, s = x - ti;
  const double d = (y1 - y0) / h;
  const double c2 = (3 * d - 2 * m0 - m1) / h, c3 = (m0 + m1 - 2 * d) / (h * h);
  return y0 + s * (m0 + s * (c2 + s * c3));
}

// the value of one component at `time` (clamped to the breaks' range)
IDTO_MPC_HD inline double spline_value(const double* t, int n, const double* y, const double* m, int stride, double time) {
  const int i = spline_interval(t, n, &time);
  const long long a = (long long)i * stride, b = (long long)(i + 1) * stride;
  return spline_piece(t[i], t[i + 1], y[a], y[b], m[a], m[b], time);
}

}  // namespace idto_spline
