"""The host half of the image upload (mp-mvs_amd/csrc/pm_stage.hpp: staging plan, row dealer, the row work of both entries) needs
no GPU: tests/stage_cpu_main.cpp is built with g++ from that header alone and stages into malloc'ed buffers, comparing every
byte with a naive copy."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_staging_plan_and_row_work(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler (g++) to build tests/stage_cpu_main.cpp with")
    exe = str(tmp_path / "stage_cpu")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "mp-mvs_amd", "csrc"),
                            os.path.join(ROOT, "tests", "stage_cpu_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1].startswith("ok:"), run.stdout
