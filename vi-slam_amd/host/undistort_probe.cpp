// undistort_probe.cpp -- vi::CameraModel's rectification surface (src/CameraModel.cpp:84-105) on a calibration XML: writes GetMap1 / GetMap2
// and the Undistort of a raw in_width x in_height frame to files, and prints GetK(); tests/test_rectify_gpu.py compares them with the
// library's tables and vis_rectify_host.  Undistort needs the device.
#include <cstdio>
#include <vector>
#include "vislam_host.hpp"
static bool write_file(const std::string& path, const void* p, size_t n) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, n, f) == n;
    return std::fclose(f) == 0 && ok;
}
int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: undistort_probe calibration.xml frame.raw outdir\n"); return 2; }
    vi::CameraModel m;
    m.GetCameraModel(argv[1]);
    const std::string out = argv[3];
    const cv::Mat& K = m.GetK();
    const cv::Mat &m1 = m.GetMap1(), &m2 = m.GetMap2();
    const int iw = m.GetInputWidth(), ih = m.GetInputHeight();
    cv::Mat img(ih, iw, CV_8UC1);
    FILE* f = std::fopen(argv[2], "rb");
    if (!f || std::fread(img.data, 1, (size_t)iw * ih, f) != (size_t)iw * ih) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    std::fclose(f);
    cv::Mat rect;
    m.Undistort(img, rect);
    if (!write_file(out + "/map1.bin", m1.data, m1.step * m1.rows) || !write_file(out + "/map2.bin", m2.data, m2.step * m2.rows) ||
        !write_file(out + "/undistort.bin", rect.data, rect.step * rect.rows)) { std::fprintf(stderr, "cannot write to %s\n", argv[3]); return 2; }
    std::printf("{\"valid\": %d, \"K\": [%.9g, %.9g, %.9g, %.9g], \"map1\": [%d, %d, %d], \"map2\": [%d, %d, %d], \"undistort\": [%d, %d]}\n",
                m.IsValid() ? 1 : 0, K.at<float>(0, 0), K.at<float>(1, 1), K.at<float>(0, 2), K.at<float>(1, 2), m1.rows, m1.cols, m1.type(),
                m2.rows, m2.cols, m2.type(), rect.rows, rect.cols);
    return 0;
}
