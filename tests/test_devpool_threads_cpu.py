"""The device pool under eight host threads, on the CPU and under ThreadSanitizer: flo_amd/csrc/devpool.cpp is one pool for
all the contexts of a process, so it is where the threads of a one-context-per-thread program meet. The program is
tests/native/devpool_threads_test.cpp (its head says what it checks), built here with g++ against the five-call stand-in
for the HIP runtime under tests/native/hipstub. A stand-alone program: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devpool_under_eight_threads(tmp_path):
    exe = str(tmp_path / "devpool_threads_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-pthread",
                    "-I", os.path.join(ROOT, "tests", "native", "hipstub"), "-I", os.path.join(ROOT, "flo_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "devpool_threads_test.cpp"), os.path.join(ROOT, "flo_amd", "csrc", "devpool.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("ok"), r.stdout
