"""The shape of a finished file on CPU: flo_amd/csrc/file_layout.hpp (header and TOC sizes, the frames of a lossy clip, the
placement of a file in front of its aligned DATA chunk, packed offsets, META and bit depth on the way out) against the
cases of tests/native/file_layout_test.cpp, built here with g++, sanitizers on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_file_layout_native(tmp_path):
    exe = str(tmp_path / "file_layout_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "file_layout_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.startswith("ok"), r.stdout
