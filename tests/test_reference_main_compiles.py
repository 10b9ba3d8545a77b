"""what the reference's own src/main_vi_slamGPU.cpp needs in order to build against the compat tree
(vi-slam_amd/host/compat: the reference's header names over the adapter classes, empty stand-ins for the five ROS headers it includes
without using, DataReader / VisualizerMarker stand-ins for the two out-of-scope components, forwarders for opencv2/{core,highgui,
calib3d}.hpp and a small cv::CommandLineParser) and the C-ABI library.  The reference tree is not part of this repository: the headers
that file includes are pinned in tests/golden/reference_main.json (tests/golden/make_reference_fixtures.py), and every one of them must
resolve inside the compat tree.  host/main_calls_gpu.cpp stays the runnable twin whose per-frame records the GPU parity test reads."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vi-slam_amd", "host")
REF_MAIN = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_main.json")))


def test_every_header_the_reference_main_includes_resolves_inside_the_compat_tree():
    incs = REF_MAIN["includes"]
    project = [i for i in incs if "/" in i or i.endswith(".hpp") or i.endswith(".h")]
    assert len(project) >= 13, project
    missing = [i for i in project if not os.path.exists(os.path.join(HOST, "compat", i))]
    assert not missing, missing


def test_command_line_parser_stand_in(tmp_path):
    """cv::CommandLineParser as main_vi_slamGPU.cpp:26-39,50-54 uses it: keys string, has("help"), get<string>(name)"""
    src = tmp_path / "clp.cpp"
    src.write_text('''#include "opencv2/core.hpp"
#include <cstdio>
int main(int argc, char** argv) {
    const cv::String keys = "{help h usage ? |      | print this message   }" "{gtFile     |       |  groundtruth file} " "{n | 7 | count} ";
    cv::CommandLineParser p(argc, argv, keys);
    std::printf("%d|%s|%d\\n", (int)p.has("help"), p.get<std::string>("gtFile").c_str(), p.get<int>("n"));
    return 0; }''')
    exe = str(tmp_path / "clp")
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(HOST, "compat"), str(src), "-o", exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    run = lambda *a: subprocess.run([exe, *a], capture_output=True, text=True, timeout=30).stdout.strip()      # noqa: E731
    assert run() == "0||7"
    assert run("-gtFile=/a/b.csv", "--n=12") == "0|/a/b.csv|12"
    assert run("-h") == "1||7" and run("--usage", "-gtFile=x") == "1|x|7"
