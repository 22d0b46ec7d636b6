// Triangulation of atlas tracks from known camera poses: the arithmetic shared by the host routine (triangulate.hip) and the GPU
// kernels (triangulate_gpu.hip).  As in absolute_pose_core.h, every function here is compiled for both sides from this one text, fp64,
// without FMA contraction, and uses + - * / and sqrt only (correctly rounded on both sides), so that host and device take identical
// decisions and produce identical bits.  The rule is stated in include/loftr_hip.h and DESIGN §16; the checks of the track table and
// its error bits are tracks_core.h's.
//
// Every rejection below is written as "unless (x > y)" rather than "if (x <= y)": a NaN (a non-finite pixel, a zero ray) then rejects.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "tracks_core.h"

#pragma clang fp contract(off)

#define TRI_HD __host__ __device__ inline

namespace tri {

constexpr int kMaxHyp = 64;                // hypothesis pairs enumerated per track
constexpr int kGnIters = 5;                // Gauss-Newton steps of one fit
constexpr int kRefitRounds = 4;            // the fit is repeated on the adopted point's inliers while it strictly gains inliers
constexpr int kCam = 24;                   // doubles per image of the camera table: P [3,4], centre [3], M = R^T K^-1 [3,3]
constexpr int kCounts = 8;                 // counts[0..4]: tracks per status, [5]: error bits, [6]: inlier observations of ok tracks, [7]: 0
constexpr double kParallel = 1e-12;        // den <= kParallel * a * c: the two rays are parallel

enum : int { kOk = 0, kTooShort = 1, kNoHypothesis = 2, kSmallAngle = 3, kBadCamera = 4 };
using tracks::kBadImage;                   // error bits (counts[5])
using tracks::kBadOffsets;

TRI_HD bool fin(double x) { return fabs(x) <= 1.7976931348623157e308; }       // false for NaN and the infinities
TRI_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// ---- camera table: K [9] (fx, skew, cx, fy, cy read), T [16] camera from world (top 3 x 4 read) -> tab [24]; an invalid camera is all NaN
TRI_HD void cam_table(const double* K, const double* T, double* tab) {
  const double fx = K[0], sk = K[1], cx = K[2], fy = K[4], cy = K[5];
  bool ok = fin(fx) && fin(sk) && fin(cx) && fin(fy) && fin(cy) && fx != 0.0 && fy != 0.0;
  for (int i = 0; i < 12; ++i) ok = ok && fin(T[i]);
  for (int c = 0; c < 4; ++c) {                                     // P = K [R | t]
    tab[c] = (fx * T[c] + sk * T[4 + c]) + cx * T[8 + c];
    tab[4 + c] = fy * T[4 + c] + cy * T[8 + c];
    tab[8 + c] = T[8 + c];
  }
  for (int r = 0; r < 3; ++r) tab[12 + r] = -((T[r] * T[3] + T[4 + r] * T[7]) + T[8 + r] * T[11]);      // c = -R^T t
  // K^-1 by back substitution: y = (v - cy) / fy, x = (u - cx - skew y) / fx
  const double k00 = 1.0 / fx, k11 = 1.0 / fy, k01 = -(sk / fy) / fx, k12 = -cy / fy, k02 = -(cx + sk * k12) / fx;
  for (int r = 0; r < 3; ++r) {                                     // M = R^T K^-1
    tab[15 + 3 * r] = T[r] * k00;
    tab[16 + 3 * r] = T[r] * k01 + T[4 + r] * k11;
    tab[17 + 3 * r] = (T[r] * k02 + T[4 + r] * k12) + T[8 + r];
  }
  for (int i = 0; i < kCam; ++i) ok = ok && fin(tab[i]);
  if (!ok) for (int i = 0; i < kCam; ++i) tab[i] = __builtin_nan("");
}
TRI_HD bool cam_valid(const double* tab) { return fin(tab[0]); }

// ---- step 2: the fixed enumeration of hypothesis pairs ------------------------------------------------------------------------------
// s = 1 .. L/2, i = 0 .. L-1 (only to L/2 - 1 when 2 s = L): L (L - 1) / 2 pairs in all, the half-length round last, so that
// hypothesis h < n_pairs(L) is simply s = h / L + 1, i = h mod L.
TRI_HD int n_pairs(long L) { return L < 2 ? 0 : (L >= 12 ? kMaxHyp : (int)(L * (L - 1) / 2)); }
TRI_HD void pair_at(long L, int h, long* i, long* j) {
  const long s = h / L + 1, a = h % L, b = a + s;
  *i = a;
  *j = b >= L ? b - L : b;
}

// the observations of all tracks and what the rule needs to judge them
struct Obs {
  const double* tab;       // [n_images, 24]
  const int* image;        // [N]
  const float* xy;         // [N,2]
  double thr2, cos_min;
};

// ---- step 1: unit world ray of a pixel
TRI_HD void ray(const double* cam, double u, double v, double* d) {
  const double* M = cam + 15;
  const double x = (M[0] * u + M[1] * v) + M[2], y = (M[3] * u + M[4] * v) + M[5], z = (M[6] * u + M[7] * v) + M[8];
  const double n = sqrt((x * x + y * y) + z * z);
  d[0] = x / n; d[1] = y / n; d[2] = z / n;
}

// ---- step 3: midpoint of two rays (centres ci / cj, directions di / dj)
TRI_HD bool midpoint(const double* ci, const double* di, const double* cj, const double* dj, double cos_min, double* X) {
  const double w[3] = {ci[0] - cj[0], ci[1] - cj[1], ci[2] - cj[2]};
  const double a = dot3(di, di), b = dot3(di, dj), c = dot3(dj, dj), d = dot3(di, w), e = dot3(dj, w);
  const double den = a * c - b * b;
  if (!(den > kParallel * a * c)) return false;
  if (!(b / sqrt(a * c) <= cos_min)) return false;
  const double s = (b * e - c * d) / den, t = (a * e - b * d) / den;
  if (!(s > 0.0) || !(t > 0.0)) return false;
  for (int k = 0; k < 3; ++k) X[k] = 0.5 * ((ci[k] + s * di[k]) + (cj[k] + t * dj[k]));
  return true;
}

// ---- step 4: squared pixel distance of X in a camera; false when X is not in front of it
TRI_HD bool residual2(const double* P, const double* X, double u, double v, double* r2) {
  const double x = (dot3(P, X)) + P[3], y = (dot3(P + 4, X)) + P[7], z = (dot3(P + 8, X)) + P[11];
  if (!(z > 0.0)) return false;
  const double du = x / z - u, dv = y / z - v;
  *r2 = du * du + dv * dv;
  return true;
}
TRI_HD bool inlier_of(const Obs& o, long k, const double* X, double* r2) {
  return residual2(o.tab + (long)kCam * o.image[k], X, (double)o.xy[2 * k], (double)o.xy[2 * k + 1], r2) && *r2 <= o.thr2;
}

// point of hypothesis h of the track [o0, o0 + L)
TRI_HD bool hyp_point(const Obs& o, long o0, long L, int h, double* X) {
  long i, j;
  pair_at(L, h, &i, &j);
  const double *ci = o.tab + (long)kCam * o.image[o0 + i], *cj = o.tab + (long)kCam * o.image[o0 + j];
  double di[3], dj[3];
  ray(ci, (double)o.xy[2 * (o0 + i)], (double)o.xy[2 * (o0 + i) + 1], di);
  ray(cj, (double)o.xy[2 * (o0 + j)], (double)o.xy[2 * (o0 + j) + 1], dj);
  return midpoint(ci + 12, di, cj + 12, dj, o.cos_min, X);
}

// ---- steps 3-5: the packed word of hypothesis h: count << 32 | (0xFFFFFFFF - h); 0 = rejected
TRI_HD unsigned long long hyp_word(const Obs& o, long o0, long L, int h) {
  double X[3], r2;
  if (!hyp_point(o, o0, L, h, X)) return 0;
  long i, j;
  pair_at(L, h, &i, &j);
  unsigned cnt = 0;
  bool own = true;
  for (long k = 0; k < L; ++k) {
    const bool in = inlier_of(o, o0 + k, X, &r2);
    cnt += in;
    if (k == i || k == j) own = own && in;
  }
  if (!own) return 0;
  return ((unsigned long long)cnt << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)h);
}

// ---- step 6: Gauss-Newton on the pixel reprojection error, three unknowns -----------------------------------------------------------
// one observation's terms of J^T J (upper triangle, row-major: 00 01 02 11 12 22) and J^T r; nothing when X is not in front
TRI_HD void accum9(const double* P, const double* X, double u, double v, double* a) {
  const double x = (dot3(P, X)) + P[3], y = (dot3(P + 4, X)) + P[7], z = (dot3(P + 8, X)) + P[11];
  if (!(z > 0.0)) return;
  const double pu = x / z, pv = y / z, ru = pu - u, rv = pv - v;
  const double ju[3] = {(P[0] - pu * P[8]) / z, (P[1] - pu * P[9]) / z, (P[2] - pu * P[10]) / z};
  const double jv[3] = {(P[4] - pv * P[8]) / z, (P[5] - pv * P[9]) / z, (P[6] - pv * P[10]) / z};
  a[0] = a[0] + (ju[0] * ju[0] + jv[0] * jv[0]);
  a[1] = a[1] + (ju[0] * ju[1] + jv[0] * jv[1]);
  a[2] = a[2] + (ju[0] * ju[2] + jv[0] * jv[2]);
  a[3] = a[3] + (ju[1] * ju[1] + jv[1] * jv[1]);
  a[4] = a[4] + (ju[1] * ju[2] + jv[1] * jv[2]);
  a[5] = a[5] + (ju[2] * ju[2] + jv[2] * jv[2]);
  a[6] = a[6] + (ju[0] * ru + jv[0] * rv);
  a[7] = a[7] + (ju[1] * ru + jv[1] * rv);
  a[8] = a[8] + (ju[2] * ru + jv[2] * rv);
}
// (J^T J) step = -J^T r by elimination in a fixed order without pivoting; a non-positive pivot or a non-finite step fails
TRI_HD bool gn_solve(const double* a, double* step) {
  const double p0 = a[0];
  if (!(p0 > 0.0)) return false;
  const double l10 = a[1] / p0, l20 = a[2] / p0;
  const double p1 = a[3] - l10 * a[1];
  if (!(p1 > 0.0)) return false;
  const double m12 = a[4] - l10 * a[2];
  const double l21 = m12 / p1;
  const double p2 = (a[5] - l20 * a[2]) - l21 * m12;
  if (!(p2 > 0.0)) return false;
  const double y0 = -a[6], y1 = -a[7] - l10 * y0, y2 = (-a[8] - l20 * y0) - l21 * y1;
  const double x2 = y2 / p2, x1 = y1 / p1 - l21 * x2, x0 = (y0 / p0 - l10 * x1) - l20 * x2;
  step[0] = x0; step[1] = x1; step[2] = x2;
  return fin(x0) && fin(x1) && fin(x2);
}
// kGnIters steps from X over the observations whose bit 0 is set; the sums run sequentially in ascending observation order
TRI_HD bool gn_fit(const Obs& o, long o0, long L, const uint8_t* bits, double* X) {
  double Y[3] = {X[0], X[1], X[2]};
  for (int it = 0; it < kGnIters; ++it) {
    double a[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, step[3];
    for (long k = 0; k < L; ++k)
      if (bits[k] & 1) accum9(o.tab + (long)kCam * o.image[o0 + k], Y, (double)o.xy[2 * (o0 + k)], (double)o.xy[2 * (o0 + k) + 1], a);
    if (!gn_solve(a, step)) return false;
    for (int c = 0; c < 3; ++c) Y[c] = Y[c] + step[c];
  }
  for (int c = 0; c < 3; ++c) X[c] = Y[c];
  return true;
}
// inliers of X into bit `bit` of bits[0..L) (the other bit kept) -> their number
TRI_HD long mark(const Obs& o, long o0, long L, const double* X, uint8_t* bits, int bit) {
  long cnt = 0;
  double r2;
  for (long k = 0; k < L; ++k) {
    const bool in = inlier_of(o, o0 + k, X, &r2);
    bits[k] = (uint8_t)((bits[k] & (bit ? 1 : 2)) | ((int)in << bit));
    cnt += in;
  }
  return cnt;
}
// The refit of one track from the best hypothesis' point X: bits[0..L) (the track's slice of obs_inlier, used as the work mask) ends as
// the final 0 / 1 inlier mask, X as the final point; -> inlier count, rms = root mean squared pixel error over the final inliers.
TRI_HD long refit_track(const Obs& o, long o0, long L, double* X, uint8_t* bits, double* rms) {
  for (long k = 0; k < L; ++k) bits[k] = 0;
  long best = mark(o, o0, L, X, bits, 0);
  for (int round = 0; round < kRefitRounds; ++round) {
    double F[3] = {X[0], X[1], X[2]};
    if (best < 2 || !gn_fit(o, o0, L, bits, F)) break;
    const long cnt = mark(o, o0, L, F, bits, 1);
    if (cnt < best) break;                                          // a fit that loses inliers is dropped
    const bool grew = cnt > best;
    best = cnt;
    for (int c = 0; c < 3; ++c) X[c] = F[c];
    for (long k = 0; k < L; ++k) bits[k] = (uint8_t)(bits[k] >> 1);
    if (!grew) break;                                               // another fit only over a strictly larger inlier set
  }
  double sum = 0.0, r2;
  for (long k = 0; k < L; ++k) {
    bits[k] = (uint8_t)(bits[k] & 1);
    if (bits[k] && inlier_of(o, o0 + k, X, &r2)) sum = sum + r2;
  }
  *rms = best > 0 ? sqrt(sum / (double)best) : 0.0;
  return best;
}

// ---- step 7: cosine of the angle at X between the centres of pair h, when both of its observations are final inliers
TRI_HD bool pair_cos(const Obs& o, long o0, long L, int h, const double* X, const uint8_t* bits, double* cs) {
  long i, j;
  pair_at(L, h, &i, &j);
  if (!bits[i] || !bits[j]) return false;
  const double *ci = o.tab + (long)kCam * o.image[o0 + i] + 12, *cj = o.tab + (long)kCam * o.image[o0 + j] + 12;
  const double a[3] = {X[0] - ci[0], X[1] - ci[1], X[2] - ci[2]}, b[3] = {X[0] - cj[0], X[1] - cj[1], X[2] - cj[2]};
  const double na = dot3(a, a), nb = dot3(b, b);
  if (!(na > 0.0) || !(nb > 0.0)) return false;
  *cs = dot3(a, b) / sqrt(na * nb);
  return true;
}

// ---- what a track leaves behind (vector stores; the fp64 point rounded once)
struct Out { float* xyz; int* n_inliers; float* rms_px; float* tri_cos; uint8_t* status; };
TRI_HD void write_track(const Out& w, long t, int st, const double* X, long cnt, double rms, double min_cos, bool has_cos) {
  const float nanf_ = __builtin_nanf("");
  const bool solved = st == kOk || st == kSmallAngle;
  for (int c = 0; c < 3; ++c) w.xyz[3 * t + c] = st == kOk ? (float)X[c] : nanf_;
  w.n_inliers[t] = solved ? (int)cnt : 0;
  w.rms_px[t] = solved ? (float)rms : nanf_;
  w.tri_cos[t] = solved && has_cos ? (float)min_cos : nanf_;
  w.status[t] = (uint8_t)st;
}

}  // namespace tri
