// triangulate_probe.cpp -- vi::VISystem's Triangulate / Disparity / getProjectionMat (src/VISystem.cpp:862-923, :422-471, :1872) on one
// two-view scene: reads a float32 file {fx, fy, cx, cy, w, h, R[9] (row-major), t[3], n, p1[n][2], p2[n][2]}, seeds the residual motion
// with setGtRes(t, R), and prints what the adapter left (RotationResidual / TranslationResidual as it stored them, mapPoints,
// mapPointFlags, the summary, Disparity with RotationResCam = RotationResidual, the projection matrix of the second camera) as JSON;
// tests/test_triangulate_gpu.py compares them with vis_triangulate.  Needs the device.
#include <cstdio>
#include <vector>
#include "vislam_host.hpp"
int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: triangulate_probe scene.f32\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    float head[19];
    if (!f || std::fread(head, 4, 19, f) != 19) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    const int n = (int)head[18];
    std::vector<float> xy(4 * (size_t)std::max(n, 0));
    if (n < 0 || std::fread(xy.data(), 4, xy.size(), f) != xy.size()) { std::fprintf(stderr, "short file %s\n", argv[1]); return 2; }
    std::fclose(f);
    cv::Mat K = cv::Mat::eye(3, 3, CV_32FC1);
    K.at<float>(0, 0) = head[0]; K.at<float>(1, 1) = head[1]; K.at<float>(0, 2) = head[2]; K.at<float>(1, 2) = head[3];
    vi::VISystem sys;
    sys.InitializePyramid((int)head[4], (int)head[5], K);
    cv::Mat Rm(3, 3, CV_32FC1), tm(3, 1, CV_32FC1);
    for (int i = 0; i < 9; i++) Rm.at<float>(i / 3, i % 3) = head[6 + i];
    for (int i = 0; i < 3; i++) tm.at<float>(i, 0) = head[15 + i];
    sys.setGtRes(tm, Rm);
    sys.RotationResCam = sys.RotationResidual;
    std::vector<cv::KeyPoint> k1(n), k2(n);
    for (int i = 0; i < n; i++) { k1[i].pt.x = xy[2 * i]; k1[i].pt.y = xy[2 * i + 1]; k2[i].pt.x = xy[2 * n + 2 * i]; k2[i].pt.y = xy[2 * n + 2 * i + 1]; }
    sys.Triangulate(k1, k2);
    const float disparity = sys.Disparity(k1, k2);
    cv::Mat Rt(3, 3, CV_32FC1), nt(3, 1, CV_32FC1);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rt.at<float>(r, c) = sys.RotationResidual(c, r);
    const cv::Mat P2 = sys.getProjectionMat(K, Rt, sys.TranslationResidual);
    std::printf("{\"RotationResidual\": [");
    for (int i = 0; i < 9; i++) std::printf("%s%.9g", i ? ", " : "", sys.RotationResidual(i / 3, i % 3));
    std::printf("], \"TranslationResidual\": [%.9g, %.9g, %.9g], ", sys.TranslationResidual.at<float>(0, 0), sys.TranslationResidual.at<float>(1, 0),
                sys.TranslationResidual.at<float>(2, 0));
    std::printf("\"summary\": [%d, %d, %d, %.9g], \"disparity\": %.9g, \"projection\": [", sys.lastTriangulation.n_points, sys.lastTriangulation.n_front,
                sys.lastTriangulation.n_kept, sys.lastTriangulation.mean_parallax_px, disparity);
    for (int i = 0; i < 12; i++) std::printf("%s%.9g", i ? ", " : "", P2.at<float>(i / 4, i % 4));
    std::printf("], \"mapPoints\": [");
    for (int i = 0; i < n; i++) std::printf("%s[%.9g, %.9g, %.9g]", i ? ", " : "", sys.mapPoints[i].x, sys.mapPoints[i].y, sys.mapPoints[i].z);
    std::printf("], \"mapPointFlags\": [");
    for (int i = 0; i < n; i++) std::printf("%s%d", i ? ", " : "", (int)sys.mapPointFlags[i]);
    std::printf("]}\n");
    return 0;
}
