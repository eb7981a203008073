"""The host side of quality ladders on CPU: flo_amd/csrc/ladder_plan.cpp (the partition of a batch's clips into groups whose
scratch stays under a limit, and that scratch per frame) against the cases of tests/native/ladder_plan_test.cpp,
built here with g++, sanitizers on; the new symbols in the header, the export list and the Python package."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LADDER_SYMBOLS = ["flo_batch_encode_ladder", "flo_ladder_shape", "flo_ladder_file_bytes", "flo_ladder_fetch", "flo_ladder_device_files",
                  "flo_ladder_destroy", "flo_encode_batch_ladder"]


def test_ladder_plan_native(tmp_path):
    exe = str(tmp_path / "ladder_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "native", "ladder_plan_test.cpp"),
                    os.path.join(ROOT, "flo_amd", "csrc", "ladder_plan.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.startswith("ok"), r.stdout


def test_ladder_symbols_are_declared_listed_and_exported():
    import flo_amd
    from flo_amd import _native
    header = open(os.path.join(ROOT, "include", "flo_hip.h")).read()
    lib = _native.lib()
    for s in LADDER_SYMBOLS:
        assert re.search(r"\b%s\(" % s, header), s
        assert s in _native.EXPORTS and hasattr(lib, s), s
    assert "typedef struct flo_ladder flo_ladder;" in header
    for name in ("Ladder", "encode_ladder", "encode_ladder_many"):
        assert hasattr(flo_amd, name), name
    assert hasattr(flo_amd.Batch, "encode_ladder")


def test_cli_rungs():
    import pytest
    from flo_amd import cli
    assert cli.parse_rungs("low,medium,high,veryhigh,transparent") == [0.2, 0.4, 0.6, 0.8, 1.0]
    assert cli.parse_rungs(" High ,vh,med, trans,high") == [0.6, 0.8, 0.4, 1.0, 0.6]
    for bad in ("", "loud", "0.5", "low,,high"):
        with pytest.raises(ValueError):
            cli.parse_rungs(bad)
