"""The role map of the stereo chain encode on CPU: which wave of a workgroup serves which clip slot in which role
(flo_amd/csrc/chain2q_roles.hpp), checked by tests/native/chain2q_roles_test.cpp, built here with g++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain2q_role_map(tmp_path):
    exe = str(tmp_path / "chain2q_roles_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "chain2q_roles_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.endswith("ok\n"), r.stdout
