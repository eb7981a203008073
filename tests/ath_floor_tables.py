"""The host table builder's band map, ATH amplitude thresholds and bands' hearing floors (flo_amd/csrc/tables.cpp), read
through a small program compiled against it: what the device is handed, bit for bit."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "flo_amd", "csrc")

PROG = r"""
#include "tables.hpp"
#include "pack_rows.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) {
    flo::LossyTablesHost t;
    flo::build_lossy_tables((uint32_t)atoi(argv[1]), (float)atof(argv[2]), t);
    static_assert(sizeof(t.masks.band_ath_floor) == 32 * sizeof(float), "32 entries");
    fwrite(t.masks.band_ath_floor, sizeof(float), 32, stdout);
    fwrite(t.ath_lin.data(), sizeof(float), 1024, stdout);
    fwrite(t.band.data(), 1, 1024, stdout);
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def program():
    """path of the compiled dump program (built once per process, in a temporary directory of its own)"""
    gxx = shutil.which("g++")
    if gxx is None:
        raise RuntimeError("g++ is required to build the host table builder")
    d = tempfile.mkdtemp(prefix="ath_floor_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    src = os.path.join(d, "dump.cpp")
    with open(src, "w") as f:
        f.write(PROG)
    exe = os.path.join(d, "dump")
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, src, os.path.join(CSRC, "tables.cpp"), "-o", exe])
    return exe


@functools.lru_cache(maxsize=None)
def load(rate, quality):
    """dict(floor f32 [32], ath_lin f32 [1024], band u8 [1024]) of (rate, quality)"""
    raw = subprocess.check_output([program(), str(rate), repr(float(quality))])
    assert len(raw) == 128 + 4096 + 1024
    return dict(floor=np.frombuffer(raw[:128], np.float32), ath_lin=np.frombuffer(raw[128:128 + 4096], np.float32),
                band=np.frombuffer(raw[128 + 4096:], np.uint8))
