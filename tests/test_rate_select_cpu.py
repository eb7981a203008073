"""The candidate choice of the rate-targeted encode on CPU: flo_amd/csrc/rate_select.cpp against the table of
tests/native/rate_select_test.cpp (built here with g++, sanitizers on), and the same table through the C ABI
(flo_rate_pick via flo_amd.rate_pick: the library loads without a GPU, no context is involved)."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rate_select_native(tmp_path):
    exe = str(tmp_path / "rate_select_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "rate_select_test.cpp"),
                    os.path.join(ROOT, "flo_amd", "csrc", "rate_select.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.startswith("ok"), r.stdout


Q = [0.5, 0.125, 0.75, 0.5, 0.25, 1.0]
Z = [500, 300, 450, 480, 700, 900]
Q32 = [(31 - i) / 31 for i in range(32)]
Z32 = [1000 * (32 - i) for i in range(32)]
NAN = math.nan


@pytest.mark.parametrize("q, z, budget, want", [
    (Q, Z, 1000, (5, True)), (Q, Z, 900, (5, True)), (Q, Z, 899, (2, True)), (Q, Z, 460, (2, True)), (Q, Z, 449, (1, True)),
    (Q, Z, 300, (1, True)), (Q, Z, 299, (1, False)), (Q, Z, 0, (1, False)),
    ([0.5, 0.5, 0.25], [10, 10, 5], 10, (0, True)), ([0.5, 0.5, 0.25], [11, 10, 5], 10, (1, True)),
    ([0.5, 0.0, 0.0], [9, 8, 7], 1, (1, False)),
    ([0.3], [100], 100, (0, True)), ([0.3], [100], 99, (0, False)),
    (Q32, Z32, 32000, (0, True)), (Q32, Z32, 16500, (16, True)), (Q32, Z32, 1000, (31, True)), (Q32, Z32, 999, (31, False)),
    ([NAN, 0.1], [5, 5], 5, (1, True)), ([0.1, NAN], [50, 60], 5, (1, False)), ([0.0, NAN, 0.2], [5, 5, 50], 5, (0, True)),
    ([1.0, 2.0], [5, 5], 5, (0, True)), ([0.9, 2.0], [5, 5], 5, (1, True)), ([0.0, -1.0], [50, 50], 5, (0, False)),
    ([0.1, -1.0], [50, 50], 5, (1, False)), ([0.1, 0.2], [2 ** 64 - 1, 2 ** 64 - 2], 2 ** 64 - 2, (1, True)),
])
def test_rate_pick_through_the_abi(q, z, budget, want):
    import flo_amd
    assert flo_amd.rate_pick(q, z, budget) == want


def test_rate_pick_refuses_bad_counts():
    import flo_amd
    with pytest.raises(flo_amd.FloError):
        flo_amd.rate_pick([], [], 10)
    with pytest.raises(flo_amd.FloError):
        flo_amd.rate_pick([0.5] * 33, [1] * 33, 10)
    with pytest.raises(ValueError):
        flo_amd.rate_pick([0.5, 0.6], [1], 10)
    assert len(flo_amd.DEFAULT_RATE_GRID) == 17 and flo_amd.DEFAULT_RATE_GRID[0] == 0.0 and flo_amd.DEFAULT_RATE_GRID[-1] == 1.0
    assert all(flo_amd.DEFAULT_RATE_GRID[i] == i / 16 for i in range(17))
