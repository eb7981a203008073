"""The band table as lane masks (StatMasks in flo_amd/csrc/pack_rows.h, built by tables.cpp), which the lock-step stereo chain
kernel's band statistics use instead of rows kRowKeep / kRowDst, against those rows and the slot lists, on the host:

    close[e]    bit l set exactly where lane l's kRowKeep value at element e is 0.0; the dirty bitmap is the set of non-empty
                masks; every lane closes behind element 15 (the kernel stores there without a mask)
    slots       walking the elements with one running slot number per lane, started at lane_slot0 and advanced behind every
                close, gives exactly kRowDst's segment slots (and kRowDst's other entries are the lanes' trash slots): the
                slot lists kRowLst / kRowLstCold / pack_ext therefore name the same (lane, segment) sequences in both forms
    gather[g]   bit l set exactly where lane l's list has more than 4 g entries in front of its zero-slot padding
    capacity    every slot number stays below kSlotCap
"""
import os
import re
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
    const int head[10] = {flo::kPackRows, flo::kRowKeep, flo::kRowDst, flo::kRowLst, flo::kRowLstCold, flo::kRowLane,
                          flo::kMaxSlots, t.n_slots, (int)t.dirty, (int)t.masks_ok};
    fwrite(head, sizeof(int), 10, stdout);
    fwrite(t.masks.close, 8, 16, stdout);
    fwrite(t.masks.gather, 8, 3, stdout);
    fwrite(t.lane_slot0.data(), 4, 64, stdout);
    fwrite(t.pack.data(), sizeof(float), t.pack.size(), stdout);
    fwrite(t.pack_ext.data(), sizeof(float), t.pack_ext.size(), stdout);
    return 0;
}
"""

RATES = [8000, 11025, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 128000, 176400, 192000]


@pytest.fixture(scope="module")
def tables_prog(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is required to build the host table builder")
    d = tmp_path_factory.mktemp("stat_masks")
    src = d / "dump.cpp"
    src.write_text(PROG)
    exe = d / "dump"
    subprocess.check_call([gxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src),
                           os.path.join(CSRC, "tables.cpp"), "-o", str(exe)])
    return str(exe)


def load(exe, rate, quality=0.55):
    raw = subprocess.check_output([exe, str(rate), str(quality)])
    head = np.frombuffer(raw[:40], dtype=np.int32)
    names = ("rows", "keep", "dst", "lst", "cold", "lane", "cap", "n_slots", "dirty", "ok")
    t = dict(zip(names, (int(v) for v in head)))
    p = 40
    t["close"] = [int(v) for v in np.frombuffer(raw[p:p + 128], dtype=np.uint64)]
    t["gather"] = [int(v) for v in np.frombuffer(raw[p + 128:p + 152], dtype=np.uint64)]
    p += 152
    t["first"] = np.frombuffer(raw[p:p + 256], dtype=np.uint32)
    p += 256
    n = t["rows"] * 64 * 16
    t["pack"] = np.frombuffer(raw[p:p + n], dtype=np.uint32).reshape(t["rows"], 64, 4)
    t["ext"] = np.frombuffer(raw[p + n:], dtype=np.uint32).reshape(2, 64, 4)
    return t


def lane_row(t, row0, lane, n):
    """n consecutive per-lane entries starting at row row0 (four per row)"""
    return t["pack"][row0:row0 + n // 4, lane, :].reshape(-1)


def slot_list(t, lane):
    """the 32 entries of the lane's slot list as slot numbers (the kernels' three sources of it)"""
    raw = np.concatenate([lane_row(t, t["lst"], lane, 12), lane_row(t, t["cold"], lane, 12), t["ext"][:, lane, :].reshape(-1)])
    assert not (raw % 8).any()
    return raw // 8


@pytest.mark.parametrize("rate", RATES)
def test_close_masks_are_the_keep_rows(tables_prog, rate):
    for q in (0.0, 0.55, 0.99):
        t = load(tables_prog, rate, q)
        assert t["ok"] == 1
        for lane in range(64):
            keep = lane_row(t, t["keep"], lane, 16).view(np.float32)
            assert set(keep.tolist()) <= {0.0, 1.0}
            for e in range(16):
                assert ((t["close"][e] >> lane) & 1) == int(keep[e] == 0.0), (rate, lane, e)
        assert t["dirty"] == sum(1 << e for e in range(16) if t["close"][e])
        assert t["close"][15] == (1 << 64) - 1


@pytest.mark.parametrize("rate", RATES)
def test_running_slot_numbers_are_the_destination_rows(tables_prog, rate):
    t = load(tables_prog, rate)
    with open(os.path.join(CSRC, "lossy_device.hpp")) as f:
        cap = int(re.search(r"constexpr int kSlotCap = (\d+);", f.read()).group(1))
    assert cap == t["cap"] and t["n_slots"] <= cap
    assert np.array_equal(t["first"], t["pack"][t["lane"], :, 1])      # what band_stats_2_prepare reads
    nxt = [int(v) for v in t["first"]]
    owner = {}                                                          # slot -> (lane, segment)
    for e in range(16):
        for lane in range(64):
            dst = int(lane_row(t, t["dst"], lane, 16)[e])
            assert dst % 8 == 0
            if (t["close"][e] >> lane) & 1:
                assert dst // 8 == nxt[lane] < cap, (rate, lane, e)
                assert nxt[lane] not in owner
                owner[nxt[lane]] = (lane, nxt[lane] - int(t["first"][lane]))
                nxt[lane] += 1
            else:
                assert dst // 8 == cap + lane, (rate, lane, e)             # the trash slot the masked form never writes
    assert sorted(owner) == list(range(t["n_slots"]))
    # every list entry names a written slot or the zero slot; a band's slots alternate between lanes b and 32 + b in
    # slot order, and every written slot is on exactly one list: the (lane, segment) sequences summed per band
    zero = cap + 64
    seen = []
    for b in range(32):
        even = [int(s) for s in slot_list(t, b) if s != zero]
        odd = [int(s) for s in slot_list(t, 32 + b) if s != zero]
        assert all(s in owner for s in even + odd)
        merged = sorted(even + odd)
        assert even == merged[0::2] and odd == merged[1::2], (rate, b)
        seen += merged
    assert sorted(seen) == list(range(t["n_slots"]))


@pytest.mark.parametrize("rate", RATES)
def test_gather_masks_are_the_list_lengths(tables_prog, rate):
    t = load(tables_prog, rate)
    zero = t["cap"] + 64
    for lane in range(64):
        lst = slot_list(t, lane)
        n = int((lst != zero).sum())
        assert (lst[:n] != zero).all() and (lst[n:] == zero).all()      # the padding is behind the entries
        for g in range(3):
            assert ((t["gather"][g] >> lane) & 1) == int(n > 4 * g), (rate, lane, g, n)
