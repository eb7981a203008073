#!/usr/bin/env python3
"""Per-site LDS model of one stereo frame of lossy_chain2q_kernel's transform wave.

For every ds_* instruction the transform wave executes per frame (the list in sites() follows the --save-temps ISA of
the bench instantiation, lossy_chain2q_kernel<false, dirty, false>, in program order) this computes the LDS-array
cycles and the bank-conflict cycles from the lane addresses the kernel really uses: the per-lane pack rows, the FFT
exchange strides, the post-rotation transposition, the band-statistics slot destinations and gather lists (built
here exactly as tables.cpp builds them for the sample rate given), the band tables of the masking pass.

Bank rules (CDNA4 LDS, per wave instruction): an access is served in fixed lane groups, one array cycle per group when
conflict-free; within a group every extra distinct dword address on one bank costs one more cycle (identical addresses
broadcast).
  ds_read_b32, ds_write_b32/b16     2 x 32 lanes, bank = dword mod 32
  ds_read_b64                       2 x 32 lanes, bank = dword mod 64
  ds_read_b128                      4 x 16 lanes {0-3,12-15,20-27} {4-11,16-19,28-31} (+32), bank = dword mod 64
  ds_read2_b32                      two ds_read_b32
  ds_read2_b64                      two accesses, each 4 x 16 contiguous lanes, bank = dword mod 32
  ds_write_b64                      4 x 16 contiguous lanes, bank = dword mod 32
  ds_write_b128                     8 x 8 contiguous lanes, bank = dword mod 32
  ds_write2_b64                     two ds_write_b64 (assumed by analogy with ds_read2_b64; not measured by itself)
A lane group none of whose lanes is enabled is still charged its cycle (the counters of the masked band statistics,
--layout masks, agree with this reading to within two cycles per frame).

The packer wave's LDS work depends on the data (non-zeros per frame, fall-back forms); it is not modelled here: the
counters' per-frame totals minus this model's transform-wave totals are the packer's share.

  python3 diag/lds_model.py [--rate 44100] [--layout old|new|masks|carry|fftrows] [--isa lossy_kernels-hip-amdgcn-amd-amdhsa-gfx950.s]
--layout old: the pack rows as the compiler read them before pack_row() (dword pieces, read2_b64, kRowLane's rcount);
--layout new: whole-row reads, rcount from row kRowS10;
--layout masks: new, with the band statistics by lane masks (band_stats_2<., true, true>): no keep / dst rows, one
  ds_write2_b64 per dirty position below 15 that carries the closing lanes only, the last store as it was.
--layout carry: masks, with the rotation twiddles (rows kRowTw) in registers for the launch: the fold and the
  post-rotation read no twiddle row (fold_carry_2, post_rotate_transpose_2_tw).
--layout fftrows: carry, with the FFT's twiddles (rows kRowF1 / kRowF2) in registers for the launch too: the FFT reads no
  constant row (fft512_2_tw); the shipped layout.
  --gather-masks: the three gather groups under their list-length masks too (diag/exp_gather_masks.patch).
  --skip-empty charges nothing for a lane group with no enabled lane (the other reading of the hardware; the counters
  say it is the wrong one: DESIGN.md §6).
With --isa, the ds_* instruction mix of one unrolled frame of the bench kernel is read from the listing and compared
with the model's site list.
"""
import argparse
import re
from collections import Counter

import numpy as np

N, HOP, NB = 2048, 1024, 25
SLOT_CAP = 96
ROW = 1024          # bytes per pack row (64 lanes x 16 B)
EDGES = np.array([0, 100, 200, 300, 400, 510, 630, 770, 920, 1080, 1270, 1480, 1720, 2000, 2320, 2700, 3150, 3700,
                  4400, 5300, 6400, 7700, 9500, 12000, 15500, 20500], dtype=np.float32)

# pack rows (pack_rows.h)
R_WIN, R_TW, R_F1, R_F2, R_LANE, R_KEEP, R_DST, R_S10 = 0, 8, 12, 16, 20, 21, 25, 32


def bands(rate):
    res = np.float32(rate) / np.float32(N)
    band = []
    for k in range(HOP):
        f = (np.float32(k) + np.float32(0.5)) * res
        b = NB - 1
        for i in range(1, 26):
            if f < EDGES[i]:
                b = i - 1
                break
        band.append(b)
    return band


def band_tables(rate):
    """lane_bnd, lane_slot0, band_slot0, dirty as tables.cpp builds them"""
    band = bands(rate)
    lane_bnd, lane_slot0, slot_band = [0] * 64, [0] * 64, []
    for j in range(64):
        lane_slot0[j] = len(slot_band)
        for e in range(16):
            k = 16 * j + e
            if e == 15 or band[k + 1] != band[k]:
                lane_bnd[j] |= 1 << e
                slot_band.append(band[k])
    dirty = 0
    for m in lane_bnd:
        dirty |= m
    band_slot0, s = [], 0
    for b in range(NB):
        band_slot0.append(s)
        while s < len(slot_band) and slot_band[s] == b:
            s += 1
    band_slot0.append(s)
    return lane_bnd, lane_slot0, band_slot0, dirty


# ------------------------------------------------------------------------------------------------ bank rules
G128 = [[0, 1, 2, 3, 12, 13, 14, 15] + list(range(20, 28)), [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19] + list(range(28, 32))]
G128 = G128 + [[l + 32 for l in g] for g in G128]
G32 = [list(range(0, 32)), list(range(32, 64))]


def contig(n):
    return [list(range(i, i + n)) for i in range(0, 64, n)]


RULES = {   # kind: (list of accesses, each (lane groups, dwords per lane, banks))
    "ds_read_b32": [(G32, 1, 32)], "ds_write_b32": [(G32, 1, 32)], "ds_write_b16": [(G32, 1, 32)],
    "ds_read_b64": [(G32, 2, 64)], "ds_read_b128": [(G128, 4, 64)],
    "ds_read2_b32": [(G32, 1, 32), (G32, 1, 32)], "ds_write2_b32": [(G32, 1, 32), (G32, 1, 32)],
    "ds_read2_b64": [(contig(16), 2, 32), (contig(16), 2, 32)],
    "ds_write_b64": [(contig(16), 2, 32)], "ds_write_b128": [(contig(8), 4, 32)],
    "ds_write2_b64": [(contig(16), 2, 32), (contig(16), 2, 32)],
}
SKIP_EMPTY = False
GATHER_MASKS = False


def cost(kind, addrs):
    """(array cycles, conflict cycles) of one wave instruction. addrs: one byte address per lane (None = lane off), or for
    the two-address forms a pair of such lists."""
    acc = RULES[kind]
    lists = addrs if len(acc) == 2 else [addrs]
    cyc = base = 0
    for (groups, dw, nbank), ad in zip(acc, lists):
        for g in groups:
            per_bank = {}
            for l in g:
                if ad[l] is None:
                    continue
                for i in range(dw):
                    d = ad[l] // 4 + i
                    per_bank.setdefault(d % nbank, set()).add(d)
            if SKIP_EMPTY and not per_bank:
                continue
            cyc += max([len(v) for v in per_bank.values()] or [1])
            base += 1
    return cyc, cyc - base


# ------------------------------------------------------------------------------------------------ sites
def lanes(f):
    return [f(l) for l in range(64)]


def sites(rate, layout):
    lane_bnd, lane_slot0, band_slot0, dirty = band_tables(rate)
    row = lambda r, off=0: lanes(lambda l: r * ROW + 16 * l + off)
    uni = lambda a: lanes(lambda l: a)
    one = lambda a: [a] + [None] * 63
    S = []   # (phase, site, kind, addrs)
    S += [("frame", "peek consumed / coef counters", "ds_read_b32", uni(0x8000))] * 2
    S += [("frame", "kRowS10 (uniform)", "ds_read_b128", uni(R_S10 * ROW))] * 2
    if layout == "old":
        S += [("frame", "rcount: kRowLane .z", "ds_read_b32", row(R_LANE, 8))]
    else:
        S += [("frame", "rcount: kRowS10 dword 64 + lane", "ds_read_b32", lanes(lambda l: R_S10 * ROW + 256 + 4 * l))]
    for ph, rr in (("fft pass 1", R_F1), ("fft pass 2", R_F2)):
        if layout == "fftrows":   # (the eight kRowF1 / kRowF2 rows stay in registers for the launch: fft512_2_tw)
            continue
        S += [(ph, "twiddle rows", "ds_read_b128", row(rr + k)) for k in range(3)]
        S += [(ph, "twiddle row 4 (.xy)", "ds_read_b64", row(rr + 3))]
    X = 0x10000   # clip block (the offset of an instruction's common base does not change its banks)
    for ka in range(8):
        S += [("fft exchange 1", "writes", "ds_write_b128", lanes(lambda l: X + 16 * ((8 * ka + (l & 7)) * 9 + (l >> 3))))]
    for r in range(8):
        S += [("fft exchange 1", "reads", "ds_read_b128", lanes(lambda l: X + 16 * (l * 9 + r)))]
    T = X + 16000   # band tables of the masking pass: ts[par][band] float4, sfwh u16, alive
    S += [("masking pass", "ts_ready peek", "ds_read_b32", uni(0x8004))]
    S += [("masking pass", "ts (tl, sf)", "ds_write2_b32", [lanes(lambda l: T + 16 * (l & 31) + 4 * (l >> 5) + o if (l & 31) < 25 else None) for o in (0, 8)])]
    S += [("masking pass", "sfwh", "ds_write_b16", lanes(lambda l: T + 1024 + 2 * l if (l & 31) < 25 else None))]
    S += [("masking pass", "alive", "ds_write_b64", one(T + 1200))]
    S += [("masking pass", "ts_ready", "ds_write_b32", one(0x8004))]
    for kb in range(8):
        S += [("fft exchange 2", "writes", "ds_write_b128", lanes(lambda l: X + 16 * (((l >> 3) + 8 * kb) * 9 + (l & 7))))]
    for r in range(8):
        S += [("fft exchange 2", "reads", "ds_read_b128", lanes(lambda l: X + 16 * (l * 9 + r)))]
    pl = lambda l: 2 * l + 2 * (l >> 3)
    for r in range(8):
        if layout == "old" or r % 2 == 0:
            if layout == "old":
                S += [("post-rotation", "twiddle rows (half rows)", "ds_read_b64", row(R_TW + r // 2, 8 * (r & 1)))]
            elif layout not in ("carry", "fftrows"):   # (carry: the four kRowTw rows stay in registers for the launch)
                S += [("post-rotation", "twiddle rows", "ds_read_b128", row(R_TW + r // 2))]
        S += [("post-rotation", "transpose writes (2m)", "ds_write_b64", lanes(lambda l: X + 8 * (pl(l) + 144 * r)))]
        S += [("post-rotation", "transpose writes (1023-2m)", "ds_write_b64", lanes(lambda l: X + 8 * (1149 - pl(l) - 144 * r)))]
    for q in range(8):
        S += [("post-rotation", "transpose reads", "ds_read_b128", lanes(lambda l: X + 16 * (9 * l) + 16 * q))]
    S += [("band statistics", "coef_ready", "ds_write_b32", one(0x8008))]
    es = [e for e in range(16) if (dirty >> e) & 1]
    if layout == "old":
        # the keep / destination dwords of the dirty elements, in the pieces the compiler reads them (b32 / b64 / read2_b32)
        for rr in (R_KEEP, R_DST):
            for g in range(4):
                comp = [e - 4 * g for e in es if 4 * g <= e < 4 * g + 4 and (rr == R_DST or e < 15)]
                i = 0
                while i < len(comp):
                    if i + 1 < len(comp) and comp[i + 1] == comp[i] + 1 and comp[i] % 2 == 1:
                        S += [("band statistics", "keep / dst rows (dword pieces)", "ds_read2_b32", [row(rr + g, 4 * comp[i]), row(rr + g, 4 * comp[i] + 4)])]
                        i += 2
                    elif i + 1 < len(comp) and comp[i + 1] == comp[i] + 1:
                        S += [("band statistics", "keep / dst rows (dword pieces)", "ds_read_b64", row(rr + g, 4 * comp[i]))]
                        i += 2
                    else:
                        S += [("band statistics", "keep / dst rows (dword pieces)", "ds_read_b32", row(rr + g, 4 * comp[i]))]
                        i += 1
    elif layout == "new":
        S += [("band statistics", "keep / dst rows (whole rows)", "ds_read_b128", row(rr + g)) for rr in (R_KEEP, R_DST) for g in range(4)]
    SL = X + 9216
    masks = layout in ("masks", "carry", "fftrows")
    for e in es:
        def dst(l, e=e, off=0):
            m = lane_bnd[l]
            if (m >> e) & 1:
                return SL + 16 * (lane_slot0[l] + bin(m & ((1 << e) - 1)).count("1")) + off
            return None if masks else SL + 16 * (SLOT_CAP + l)   # masked off / the lane's trash slot
        if masks and e == 15:   # every lane closes its last segment: unmasked, the quad as it is
            S += [("band statistics", "slot store (element 15, all lanes)", "ds_write_b128", lanes(dst))]
        elif masks:
            S += [("band statistics", "slot stores (closing lanes)", "ds_write2_b64", [lanes(dst), lanes(lambda l: dst(l, off=8))])]
        else:
            S += [("band statistics", "slot stores", "ds_write_b128", lanes(dst))]
    zero = SLOT_CAP + 64
    for u in range(12):
        def src(l, u=u):
            b = min(l & 31, 24)
            bs0 = band_slot0[b] + (l >> 5)
            bs1 = band_slot0[b + 1] if (l & 31) < 25 else 0
            s = bs0 + 2 * u
            if masks and GATHER_MASKS and not bs0 + 2 * 4 * (u // 4) < bs1:
                return None   # the lane's list ends before this group
            return SL + 16 * (s if s < bs1 else zero)
        S += [("band statistics", "slot gathers", "ds_read_b128", lanes(src))]
    for r in range(8):
        S += [("fold", "window rows", "ds_read_b128", row(R_WIN + r))]
    if layout == "old":
        for k in range(4):
            S += [("fold", "twiddle rows (read2_b64)", "ds_read2_b64", [row(R_TW + k), row(R_TW + k, 8)])]
    elif layout not in ("carry", "fftrows"):
        S += [("fold", "twiddle rows", "ds_read_b128", row(R_TW + k)) for k in range(4)]
    return S


def isa_mix(path):
    """ds_* mix of the first unrolled frame of the bench instantiation's transform loop (lossy_chain2q_kernel<false, d,
    false> with d != 65535): from the frame loop's header (the last '%.lr.ph' block in front of the frame body's end label) to the block behind that label. The runtime loop over gather groups >= 3 (from the first branch
    to the frame body's end label on) does not run at 44.1 kHz and is reported apart."""
    txt = open(path).read().split("\n")
    start = next(i for i, t in enumerate(txt) if re.match(r"^_ZN3flo20lossy_chain2q_kernelILb0ELj(\d+)ELb0EE.*:", t)
                 and "Lj65535E" not in t)
    body = txt[start:]
    e = next(i for i, t in enumerate(body) if re.match(r"^\.LBB\d+_\d+:.*_clEjS\d_S\d_S\d_S\d_\.exit", t))
    a = max(i for i, t in enumerate(body[:e]) if re.match(r"^\.LBB\d+_\d+:\s+; %\.lr\.ph\d*$", t))
    lab = body[e].split(":")[0]
    c = next(i for i, t in enumerate(body) if i > a and re.search(r"s_cbranch\w*\s+" + re.escape(lab) + r"\b", t))
    b = next(i for i, t in enumerate(body) if i > e and re.match(r"^\.LBB", t))
    mix, cold = Counter(), Counter()
    for i in range(a, b):
        m = re.search(r"\b(ds_[a-z0-9_]+)", body[i])
        if m:
            (cold if c <= i < e else mix)[m.group(1)] += 1
    return mix, cold


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--layout", default="old", choices=["old", "new", "masks", "carry", "fftrows"])
    ap.add_argument("--skip-empty", action="store_true")
    ap.add_argument("--gather-masks", action="store_true")
    ap.add_argument("--isa")
    a = ap.parse_args()
    global SKIP_EMPTY, GATHER_MASKS
    SKIP_EMPTY, GATHER_MASKS = a.skip_empty, a.gather_masks
    S = sites(a.rate, a.layout)
    tab = {}
    tot_c = tot_x = 0
    for ph, site, kind, ad in S:
        c, x = cost(kind, ad)
        k = (ph, site, kind)
        n, cc, xx = tab.get(k, (0, 0, 0))
        tab[k] = (n + 1, cc + c, xx + x)
        tot_c += c
        tot_x += x
    print(f"{'phase':16} {'site':38} {'instruction':14} {'n':>3} {'array':>6} {'conflict':>8}")
    for (ph, site, kind), (n, c, x) in tab.items():
        print(f"{ph:16} {site:38} {kind:14} {n:3d} {c:6d} {x:8d}")
    print(f"{'transform wave, one stereo frame':70} {len(S):3d} {tot_c:6d} {tot_x:8d}")
    if a.isa:
        mix, cold = isa_mix(a.isa)
        model = Counter(kind for _, _, kind, _ in S)
        print("ISA mix (one frame):", dict(sorted(mix.items())), " cold loop (not run at this rate):", dict(cold))
        print("model mix          :", dict(sorted(model.items())))


if __name__ == "__main__":
    main()
