// se3_core.h -- Sophus::SE3f value operations as host + device code: the alignment kernel (align.hip), the trajectory chain
// (track.hip) and the host-side vis_se3_* helpers of the adapters all run THIS code, compiled with -ffp-contract=off, so a pose
// composed on the device equals the one composed on the host byte for byte.
#ifndef VIS_SE3_CORE_H
#define VIS_SE3_CORE_H
#include "vis_internal.h"

#define HD __host__ __device__ inline              // the SE3 pieces also back the host-side vis_se3_* helpers of the adapters

// ---- Sophus::SE3f pieces (see oracle/align.cpp for the citations) -------------------------------------------
struct Quat { float w, x, y, z; };
struct Se3 { Quat q; float t[3]; };

// deterministic double sin/cos, identical to detect.hip's / the oracle's sincos_det
HD void al_sincos(double x, double* s, double* c) {
    const double TWO_OVER_PI = 6.36619772367581382433e-01;
    const double PIO2_HI = 1.57079632673412561417e+00;
    const double PIO2_LO = 6.07710050650619224932e-11;
    const double kd = rint(x * TWO_OVER_PI);
    const int k = (int)kd;
    const double r = (x - kd * PIO2_HI) - kd * PIO2_LO;
    const double z = r * r;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
                 S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
                 S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
                 C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
                 C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double ps = S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6))));
    const double sr = r + (r * z) * ps;
    const double pc = C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))));
    const double cr = (1.0 - 0.5 * z) + (z * z) * pc;
    switch (k & 3) {
        case 0: *s = sr;  *c = cr;  break;
        case 1: *s = cr;  *c = -sr; break;
        case 2: *s = -sr; *c = -cr; break;
        default: *s = -cr; *c = sr; break;
    }
}
HD float sin_det(float a) { double s, c; al_sincos((double)a, &s, &c); return (float)s; }
HD float cos_det(float a) { double s, c; al_sincos((double)a, &s, &c); return (float)c; }

HD Quat qmul(const Quat& a, const Quat& b) {
    Quat r;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    return r;
}
HD void qrot(const Quat& q, const float (&v)[3], float (&out)[3]) {
    float uv0 = q.y * v[2] - q.z * v[1], uv1 = q.z * v[0] - q.x * v[2], uv2 = q.x * v[1] - q.y * v[0];
    uv0 += uv0; uv1 += uv1; uv2 += uv2;
    const float c0 = q.y * uv2 - q.z * uv1, c1 = q.z * uv0 - q.x * uv2, c2 = q.x * uv1 - q.y * uv0;
    out[0] = v[0] + q.w * uv0 + c0;
    out[1] = v[1] + q.w * uv1 + c1;
    out[2] = v[2] + q.w * uv2 + c2;
}
HD void qmat(const Quat& q, float (&R)[9]) {
    const float tx = 2.f * q.x, ty = 2.f * q.y, tz = 2.f * q.z;
    const float twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const float txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const float tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1.f - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
    R[3] = txy + twz;         R[4] = 1.f - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.f - (txx + tyy);
}
HD Se3 se3_exp(const float (&a)[6]) {
    const float o0 = a[3], o1 = a[4], o2 = a[5];
    const float theta_sq = o0 * o0 + o1 * o1 + o2 * o2;
    const float theta = sqrtf(theta_sq);
    const float half = 0.5f * theta;
    float imag, real;
    const float eps = 1e-5f;
    if (theta < eps) {
        const float po4 = theta_sq * theta_sq;
        imag = 0.5f - (float)(1.0 / 48.0) * theta_sq + (float)(1.0 / 3840.0) * po4;
        real = 1.f - (float)(1.0 / 8.0) * theta_sq + (float)(1.0 / 384.0) * po4;
    } else {
        imag = sin_det(half) / theta;
        real = cos_det(half);
    }
    Se3 r;
    r.q.w = real; r.q.x = imag * o0; r.q.y = imag * o1; r.q.z = imag * o2;
    const float O[9] = {0.f, -o2, o1, o2, 0.f, -o0, -o1, o0, 0.f};
    float O2[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) O2[3 * i + j] = O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j] + O[3 * i + 2] * O[6 + j];
    float V[9];
    if (theta < eps) qmat(r.q, V);
    else {
        const float ca = (1.f - cos_det(theta)) / theta_sq;
        const float cb = (theta - sin_det(theta)) / (theta_sq * theta);
#pragma unroll
        for (int i = 0; i < 9; i++) V[i] = ((i % 4 == 0) ? 1.f : 0.f) + ca * O[i] + cb * O2[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) r.t[i] = V[3 * i] * a[0] + V[3 * i + 1] * a[1] + V[3 * i + 2] * a[2];
    return r;
}
HD Se3 se3_mul(const Se3& a, const Se3& b) {
    Se3 r = a;
    float rt[3];
    qrot(a.q, b.t, rt);
    r.t[0] = a.t[0] + rt[0]; r.t[1] = a.t[1] + rt[1]; r.t[2] = a.t[2] + rt[2];
    r.q = qmul(a.q, b.q);
    const float sn = r.q.w * r.q.w + r.q.x * r.q.x + r.q.y * r.q.y + r.q.z * r.q.z;
    if (sn != 1.f) { const float s = 2.f / (1.f + sn); r.q.w *= s; r.q.x *= s; r.q.y *= s; r.q.z *= s; }
    return r;
}

// the C ABI's storage order (x, y, z, w, t) <-> the pieces above
HD Se3 to_se3(const vis_se3f& a) { Se3 r; r.q.w = a.qw; r.q.x = a.qx; r.q.y = a.qy; r.q.z = a.qz; r.t[0] = a.tx; r.t[1] = a.ty; r.t[2] = a.tz; return r; }
HD void from_se3(const Se3& e, vis_se3f* o) { o->qx = e.q.x; o->qy = e.q.y; o->qz = e.q.z; o->qw = e.q.w; o->tx = e.t[0]; o->ty = e.t[1]; o->tz = e.t[2]; }

// SE3(Matrix3 R, Point t): Eigen's rotation-matrix -> quaternion conversion (HD: the trajectory chain of track.hip runs it too)
HD void se3_from_rt_f(const float* R, const float* t, vis_se3f* out) {
    float qw, v[3];
    float tr = R[0] + R[4] + R[8];
    if (tr > 0.f) {
        tr = sqrtf(tr + 1.f);
        qw = 0.5f * tr;
        tr = 0.5f / tr;
        v[0] = (R[7] - R[5]) * tr; v[1] = (R[2] - R[6]) * tr; v[2] = (R[3] - R[1]) * tr;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        tr = sqrtf(R[4 * i] - R[4 * j] - R[4 * k] + 1.f);
        v[i] = 0.5f * tr;
        tr = 0.5f / tr;
        qw = (R[3 * k + j] - R[3 * j + k]) * tr;
        v[j] = (R[3 * j + i] + R[3 * i + j]) * tr;
        v[k] = (R[3 * k + i] + R[3 * i + k]) * tr;
    }
    out->qx = v[0]; out->qy = v[1]; out->qz = v[2]; out->qw = qw; out->tx = t[0]; out->ty = t[1]; out->tz = t[2];
}
#endif
