"""The per-lane constant pack (flo_amd/csrc/tables.cpp, rows in pack_rows.h) on the host: row kRowS10 carries, besides the
spreading levels the masking pass reads uniformly, a contiguous copy of kRowLane's per-lane 1 / bins that the stereo
chain kernel reads instead of kRowLane .z. The copy must equal the original bit for bit at every sample rate, and the
rest of the row must be what it was."""
import os
import shutil
import subprocess

import numpy as np
import pytest

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
    fwrite(&flo::kPackRows, sizeof(int), 1, stdout);
    const int rows[2] = {flo::kRowLane, flo::kRowS10};
    fwrite(rows, sizeof(int), 2, stdout);
    fwrite(t.pack.data(), sizeof(float), t.pack.size(), stdout);
    fwrite(t.s10d.data(), sizeof(float), t.s10d.size(), stdout);
    return 0;
}
"""

RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 128000, 176400, 192000]


@pytest.fixture(scope="module")
def tables_prog(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is required to build the host table builder")
    d = tmp_path_factory.mktemp("pack_rows")
    src = d / "dump.cpp"
    src.write_text(PROG)
    exe = d / "dump"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src),
                           os.path.join(CSRC, "tables.cpp"), "-o", str(exe)])
    return str(exe)


def load(exe, rate, quality):
    raw = subprocess.check_output([exe, str(rate), str(quality)])
    n_rows, r_lane, r_s10 = np.frombuffer(raw[:12], dtype=np.int32)
    pack = np.frombuffer(raw[12:12 + n_rows * 64 * 16], dtype=np.uint32).reshape(n_rows, 64, 4)
    s10d = np.frombuffer(raw[12 + n_rows * 64 * 16:], dtype=np.uint32)
    return pack, int(r_lane), int(r_s10), s10d


@pytest.mark.parametrize("rate", RATES)
def test_s10_row_holds_rcount_copy(tables_prog, rate):
    for q in (0.0, 0.55, 0.99):
        pack, r_lane, r_s10, s10d = load(tables_prog, rate, q)
        row = pack[r_s10].reshape(-1)            # 256 dwords
        assert np.array_equal(row[0:24], s10d[1:25])                 # spreading levels, read uniformly
        assert not row[24:64].any()                                  # unused
        assert np.array_equal(row[64:128], pack[r_lane, :, 2])       # 1 / bins per lane, bit for bit
        assert not row[128:].any()
        # lanes b and 32 + b carry band b's value (lanes from 25 on repeat band 24)
        rc = row[64:128].view(np.float32)
        assert np.array_equal(rc[:32], rc[32:])
        assert np.all(rc[25:32] == rc[24])
