// h_transfer.h -- the adjugate and the division-free transfer of the homography contract (include/vislam_hip.h), shared by the RANSAC
// (homography.hip) and the polish (homography_polish.hip): one copy, so both see the same bits.
#pragma once
#include "ransac_lanes.h"

// adj(M) of a row-major 3 x 3: rows c1 x c2, c2 x c0, c0 x c1 of M's columns
DEV void h_adj(const double (&M)[9], double (&G)[9]) {
    const double c0[3] = {M[0], M[3], M[6]}, c1[3] = {M[1], M[4], M[7]}, c2[3] = {M[2], M[5], M[8]};
    double r0[3], r1[3], r2[3];
    cross3(c1, c2, r0); cross3(c2, c0, r1); cross3(c0, c1, r2);
    G[0] = r0[0]; G[1] = r0[1]; G[2] = r0[2]; G[3] = r1[0]; G[4] = r1[1]; G[5] = r1[2]; G[6] = r2[0]; G[7] = r2[1]; G[8] = r2[2];
}

// (e, w w) of the transfer of (x, y, 1) by M against (u, v): the point passes at threshold t iff e <= t (w w)
DEV void h_transfer(const double (&M)[9], double x, double y, double u, double v, double& e, double& ww) {
    const double U = (M[0] * x + M[1] * y) + M[2], V = (M[3] * x + M[4] * y) + M[5], w = (M[6] * x + M[7] * y) + M[8];
    const double du = U - u * w, dv = V - v * w;
    e = du * du + dv * dv;
    ww = w * w;
}
