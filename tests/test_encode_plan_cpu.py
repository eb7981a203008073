"""The encode plan on CPU: which kernels a lossy batch encode and finish_files launch (flo_amd/csrc/encode_plan.cpp),
pinned as tables and checked for its invariants by tests/native/encode_plan_test.cpp, built here with g++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_encode_plan_tables_and_invariants(tmp_path):
    exe = str(tmp_path / "encode_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "encode_plan_test.cpp"),
                    os.path.join(ROOT, "flo_amd", "csrc", "encode_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.startswith("ok"), r.stdout
