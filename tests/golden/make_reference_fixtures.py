#!/usr/bin/env python3
"""Regenerates the fixtures that pin the repository against the reference (MecatronicaUSB/vi-slam) without the reference tree
being present: `python tests/golden/make_reference_fixtures.py REFERENCE_DIR`.

  reference_main.json      for src/main_vi_slamGPU.cpp: the file's sha256, the headers it #includes, and the sha256 of every line range
                           that vi-slam_amd/host/main_calls_gpu.cpp holds verbatim (BEGIN/END markers).  Names and digests only, no source.
  calibrationEUROC.xml     the EuRoC calibration file the reference ships (data), read by tests/test_host_adapters_gpu.py
"""
import hashlib
import json
import os
import re
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TWIN = os.path.join(ROOT, "vi-slam_amd", "host", "main_calls_gpu.cpp")


def block_digest(lines):
    """sha256 of a line range, trailing white space of every line stripped (what the verbatim check compares)"""
    return hashlib.sha256("\n".join(x.rstrip() for x in lines).encode()).hexdigest()


def verbatim_ranges(twin_text):
    return [(int(a), int(b)) for a, b in re.findall(r"// BEGIN verbatim src/main_vi_slamGPU.cpp:(\d+)-(\d+)", twin_text)]


def main(ref):
    src = open(os.path.join(ref, "src", "main_vi_slamGPU.cpp")).read()
    rl = src.split("\n")
    out = {"file": "src/main_vi_slamGPU.cpp", "sha256": hashlib.sha256(src.encode()).hexdigest(),
           "includes": re.findall(r'^\s*#include\s*[<"]([^>"]+)[>"]', src, flags=re.M),
           "verbatim_blocks": {f"{a}-{b}": block_digest(rl[a - 1:b]) for a, b in verbatim_ranges(open(TWIN).read())}}
    with open(os.path.join(HERE, "reference_main.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    shutil.copyfile(os.path.join(ref, "calibration", "calibrationEUROC.xml"), os.path.join(HERE, "calibrationEUROC.xml"))


if __name__ == "__main__":
    main(sys.argv[1])
