"""The segment fold of the packed kernel (tinykvpp_amd/csrc/tkv_crc32_fold.h) on the host: the same
header the device compiles, checked by tests/cpp/test_fold_segment.cpp against frankie::core's CRC-32
arithmetic. Needs no GPU and no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_fold_segment.cpp")


def test_fold_segment_identity(tmp_path):
    exe = str(tmp_path / "test_fold_segment")
    subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-Werror", "-Wconversion",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tinykvpp_amd", "csrc"),
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "ALL PASSED" in r.stdout
