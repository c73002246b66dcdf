// pm_align_host.hpp -- host half of the alignment (mpmvs_align_solve, the stop rule of mpmvs_align_icp).
// Umeyama's closed form ("Least-squares estimation of transformation parameters between two point patterns", PAMI 1991) in
// fp64 on the 18 integer sums of pm_align.hpp, in their normalised frame:
//   n = sums[0], s = 2^-30;  mu_a = sums[1..3] s / n,  mu_b = sums[4..6] s / n;
//   Sigma[r][c] = sums[7 + 3 c + r] s / n - mu_b[r] mu_a[c]   (target rows, source columns);  var_a = sums[16] s / n - |mu_a|^2;
//   Sigma = U diag(d) V^T by one-sided Jacobi (Hestenes) rotations, d descending; S = diag(1, 1, det(U) det(V));
//   R = U S V^T,  c = (d0 + d1 + S22 d2) / var_a with scale, else 1,  t = mu_b - c R mu_a.
// In world units the update is D = [c R | o - c R o + u t], and M_out = D * M_in.  rmse = sqrt(sums[17] s / n) * u: the RMS
// distance of the matched pairs BEFORE the update.
// Returns 1 with M_out = M_in when n < 3, var_a <= 0 or d0 == 0; anything else is answered as the formula gives it.  Collinear
// pairs (d1 == 0) leave the rotation about their line open: some rotation of that family is returned, and telling is the caller's job.
// Below it the step of point-to-plane ICP (mpmvs_align_plane_solve) on the 38 sums of pm_align_plane.hpp.
// No device code and no HIP header: plain C++.
#pragma once

#include <cmath>

namespace pm {

inline double align_det3(const double m[3][3]) {
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// a = U diag(d) V^T with d[0] >= d[1] >= d[2] >= 0, U and V orthogonal (U completed by cross products where a loses rank)
inline void align_svd3(const double a[3][3], double U[3][3], double d[3], double V[3][3]) {
    double g[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) g[r][c] = a[r][c], V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = 0; r < 3; ++r) al += g[r][p] * g[r][p], be += g[r][q] * g[r][q], ga += g[r][p] * g[r][q];
                if (ga == 0.0 || std::fabs(ga) <= 0x1p-53 * std::sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
                for (int r = 0; r < 3; ++r) {
                    const double gp = g[r][p], gq = g[r][q], vp = V[r][p], vq = V[r][q];
                    g[r][p] = cs * gp - sn * gq, g[r][q] = sn * gp + cs * gq;
                    V[r][p] = cs * vp - sn * vq, V[r][q] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
    for (int c = 0; c < 3; ++c) d[c] = std::sqrt((g[0][c] * g[0][c] + g[1][c] * g[1][c]) + g[2][c] * g[2][c]);
    for (int c = 0; c < 2; ++c)   // columns by descending norm
        for (int e = c + 1; e < 3; ++e)
            if (d[e] > d[c]) {
                const double td = d[c];
                d[c] = d[e], d[e] = td;
                for (int r = 0; r < 3; ++r) {
                    const double tg = g[r][c], tv = V[r][c];
                    g[r][c] = g[r][e], g[r][e] = tg;
                    V[r][c] = V[r][e], V[r][e] = tv;
                }
            }
    double u0[3] = {1, 0, 0}, u1[3], u2[3];
    if (d[0] > 0.0)
        for (int r = 0; r < 3; ++r) u0[r] = g[r][0] / d[0];
    // second column: what column 1 keeps orthogonal to u0; where that is lost in rounding, the axis least along u0
    double w[3], dot = 0.0, nw = 0.0;
    for (int r = 0; r < 3; ++r) dot += g[r][1] * u0[r];
    for (int r = 0; r < 3; ++r) w[r] = g[r][1] - dot * u0[r], nw += w[r] * w[r];
    nw = std::sqrt(nw);
    if (!(nw > 0x1p-40 * d[0])) {
        int k = 0;
        for (int r = 1; r < 3; ++r)
            if (std::fabs(u0[r]) < std::fabs(u0[k])) k = r;
        dot = u0[k], nw = 0.0;
        for (int r = 0; r < 3; ++r) w[r] = (r == k ? 1.0 : 0.0) - dot * u0[r], nw += w[r] * w[r];
        nw = std::sqrt(nw);
    }
    for (int r = 0; r < 3; ++r) u1[r] = w[r] / nw;
    // third column: the cross product, with the sign of column 2 (none left: +)
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1], u2[1] = u0[2] * u1[0] - u0[0] * u1[2], u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    if ((g[0][2] * u2[0] + g[1][2] * u2[1]) + g[2][2] * u2[2] < 0.0)
        for (int r = 0; r < 3; ++r) u2[r] = -u2[r];
    for (int r = 0; r < 3; ++r) U[r][0] = u0[r], U[r][1] = u1[r], U[r][2] = u2[r];
}

// the update D (row-major 3 x 4, world units) and the rmse from the sums; 1 (D = identity) in the three degenerate cases
inline int align_update(const long long sums[18], const double frame[4], int with_scale, double D[12], double* rmse) {
    for (int k = 0; k < 12; ++k) D[k] = k % 5 == 0 ? 1.0 : 0.0;
    const double n = (double)sums[0], s = 0x1p-30, u = frame[3];
    if (rmse) *rmse = sums[0] > 0 ? std::sqrt((double)sums[17] * s / n) * u : 0.0;
    if (sums[0] < 3) return 1;
    double ma[3], mb[3], sig[3][3];
    for (int k = 0; k < 3; ++k) ma[k] = (double)sums[1 + k] * s / n, mb[k] = (double)sums[4 + k] * s / n;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) sig[r][c] = (double)sums[7 + 3 * c + r] * s / n - mb[r] * ma[c];
    const double var_a = (double)sums[16] * s / n - ((ma[0] * ma[0] + ma[1] * ma[1]) + ma[2] * ma[2]);
    if (!(var_a > 0.0)) return 1;
    double U[3][3], V[3][3], d[3];
    align_svd3(sig, U, d, V);
    if (!(d[0] > 0.0)) return 1;
    const double s22 = align_det3(U) * align_det3(V) < 0.0 ? -1.0 : 1.0;
    const double c = with_scale ? ((d[0] + d[1]) + s22 * d[2]) / var_a : 1.0;
    double cR[3][3];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) cR[r][k] = c * ((U[r][0] * V[k][0] + U[r][1] * V[k][1]) + s22 * U[r][2] * V[k][2]);
    for (int r = 0; r < 3; ++r) {
        const double t = mb[r] - ((cR[r][0] * ma[0] + cR[r][1] * ma[1]) + cR[r][2] * ma[2]);
        for (int k = 0; k < 3; ++k) D[4 * r + k] = cR[r][k];
        D[4 * r + 3] = (frame[r] - ((cR[r][0] * frame[0] + cR[r][1] * frame[1]) + cR[r][2] * frame[2])) + u * t;
    }
    return 0;
}

// M_out = D * M_in, both 3 x 4 with an implied last row 0 0 0 1
inline void align_compose(const double D[12], const double M_in[12], double M_out[12]) {
    double o[12];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k)
            o[4 * r + k] = ((D[4 * r] * M_in[k] + D[4 * r + 1] * M_in[4 + k]) + D[4 * r + 2] * M_in[8 + k]) + (k == 3 ? D[4 * r + 3] : 0.0);
    for (int k = 0; k < 12; ++k) M_out[k] = o[k];
}

inline int align_solve(const long long sums[18], const double frame[4], int with_scale, const double M_in[12], double M_out[12], double* rmse) {
    double D[12];
    const int rc = align_update(sums, frame, with_scale, D, rmse);
    if (rc) {
        for (int k = 0; k < 12; ++k) M_out[k] = M_in[k];
        return rc;
    }
    align_compose(D, M_in, M_out);
    return 0;
}

// the stop rule of the ICP loop: the largest distance (Euclidean, fp64) by which D moves a corner of the box o +- u
inline double align_move(const double D[12], const double frame[4]) {
    double worst = 0.0;
    for (int c = 0; c < 8; ++c) {
        double x[3], m2 = 0.0, dd[3];
        for (int k = 0; k < 3; ++k) x[k] = (c >> k) & 1 ? frame[k] + frame[3] : frame[k] - frame[3];
        for (int k = 0; k < 3; ++k) dd[k] = (((D[4 * k] * x[0] + D[4 * k + 1] * x[1]) + D[4 * k + 2] * x[2]) + D[4 * k + 3]) - x[k];
        m2 = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2];
        const double m = std::sqrt(m2);
        worst = m > worst ? m : worst;
    }
    return worst;
}

// ---- point-to-plane (mpmvs_align_plane_solve) ----------------------------------------------------------
// One Gauss-Newton step on the 38 integer sums of pm_align_plane.hpp, in their normalised frame:
//   n = sums[0], s = 2^-30;  H = J^T J (7 x 7, symmetric, its upper triangle row by row in sums[1..28]) and gvec = J^T r
//   (sums[29..35]), both times s;  m = 7 with scale, else the leading 6;  H x = -gvec by LDL^T without pivoting, x = (omega, t, sigma).
//   Pivot j is d_j = H_jj - sum_k<j L_jk^2 d_k.  The step is refused -- 1 is returned -- for n < m, for a pivot that is not finite
//   or is <= 2^-20 H_jj (a direction the pairs do not observe: the rounding of a sum is at most n 2^-31 against a diagonal of
//   n mean(J_j^2)), and, with scale, for a 1 + sigma that is not a positive finite number.
//   R = the rotation of the unit quaternion (1, omega / 2) / |.|: proper for every omega, and it needs one sqrt only.
//   c = 1 + sigma with scale, else 1.  In world units the update is D = [c R | o - c R o + u t], as in align_update.
// rmse_plane = sqrt(sums[36] s / n) u and rmse_point = sqrt(sums[37] s / n) u: the RMS point-to-plane and point-to-point
// distance of the matched pairs BEFORE the update (0 for n = 0).
inline int align_plane_update(const long long sums[38], const double frame[4], int with_scale, double D[12], double* rmse_plane, double* rmse_point) {
    for (int k = 0; k < 12; ++k) D[k] = k % 5 == 0 ? 1.0 : 0.0;
    const double n = (double)sums[0], s = 0x1p-30, u = frame[3];
    if (rmse_plane) *rmse_plane = sums[0] > 0 ? std::sqrt((double)sums[36] * s / n) * u : 0.0;
    if (rmse_point) *rmse_point = sums[0] > 0 ? std::sqrt((double)sums[37] * s / n) * u : 0.0;
    const int m = with_scale ? 7 : 6;
    if (sums[0] < m) return 1;
    double H[7][7], L[7][7], d[7], x[7];
    for (int i = 0, k = 1; i < 7; ++i)
        for (int j = i; j < 7; ++j, ++k) H[i][j] = H[j][i] = (double)sums[k] * s;
    for (int j = 0; j < m; ++j) {
        double dj = H[j][j];
        for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k] * d[k];
        if (!std::isfinite(dj) || !(dj > 0x1p-20 * H[j][j])) return 1;
        d[j] = dj;
        for (int i = j + 1; i < m; ++i) {
            double v = H[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * d[k];
            L[i][j] = v / dj;
        }
    }
    for (int i = 0; i < m; ++i) {   // L z = -gvec
        double v = -((double)sums[29 + i] * s);
        for (int k = 0; k < i; ++k) v -= L[i][k] * x[k];
        x[i] = v;
    }
    for (int i = 0; i < m; ++i) x[i] /= d[i];
    for (int i = m - 1; i >= 0; --i)   // L^T x = z / d
        for (int k = i + 1; k < m; ++k) x[i] -= L[k][i] * x[k];
    const double c = with_scale ? 1.0 + x[6] : 1.0;
    if (!(c > 0.0) || !std::isfinite(c)) return 1;
    const double qx = 0.5 * x[0], qy = 0.5 * x[1], qz = 0.5 * x[2];
    const double qn = std::sqrt(1.0 + ((qx * qx + qy * qy) + qz * qz));
    const double w = 1.0 / qn, a = qx / qn, b = qy / qn, e = qz / qn;
    const double R[3][3] = {{1.0 - 2.0 * (b * b + e * e), 2.0 * (a * b - w * e), 2.0 * (a * e + w * b)},
                            {2.0 * (a * b + w * e), 1.0 - 2.0 * (a * a + e * e), 2.0 * (b * e - w * a)},
                            {2.0 * (a * e - w * b), 2.0 * (b * e + w * a), 1.0 - 2.0 * (a * a + b * b)}};
    for (int r = 0; r < 3; ++r) {
        const double cR[3] = {c * R[r][0], c * R[r][1], c * R[r][2]};
        for (int k = 0; k < 3; ++k) D[4 * r + k] = cR[k];
        D[4 * r + 3] = (frame[r] - ((cR[0] * frame[0] + cR[1] * frame[1]) + cR[2] * frame[2])) + u * x[3 + r];
    }
    return 0;
}

inline int align_plane_solve(const long long sums[38], const double frame[4], int with_scale, const double M_in[12], double M_out[12], double* rmse_plane,
                             double* rmse_point) {
    double D[12];
    const int rc = align_plane_update(sums, frame, with_scale, D, rmse_plane, rmse_point);
    if (rc) {
        for (int k = 0; k < 12; ++k) M_out[k] = M_in[k];
        return rc;
    }
    align_compose(D, M_in, M_out);
    return 0;
}

}  // namespace pm
