"""The flat (clip, tile) work list of the batch-to-batch operations on CPU: the tile prefix, the lookup a workgroup makes in
it and the layout of the block that carries the lists (flo_amd/csrc/clip_tiles.hpp), checked by
tests/native/clip_tiles_test.cpp, built here with g++."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clip_tiles(tmp_path):
    exe = str(tmp_path / "clip_tiles_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "clip_tiles_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.endswith("\n") and r.stdout.startswith("ok "), r.stdout
