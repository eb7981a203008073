#!/usr/bin/env python3
"""Per-clip records of a FLO_STAMPS run (FLO_STAMPS_DUMP=file): transform / packer busy ticks per frame by SIMD, XCC, slot."""
import sys
import numpy as np
st = np.fromfile(sys.argv[1], dtype=np.uint64).reshape(-1, 2, 16)
hops = int(sys.argv[2]) if len(sys.argv) > 2 else 432
t = st[:, 0, :].astype(np.float64); p = st[:, 1, :].astype(np.float64)
tb = (t[:, :9].sum(1) - t[:, 7]) / hops
pb = p[:, 1:5].sum(1) / hops
def ids(x):
    x = x.astype(np.uint64)
    hw = x & np.uint64(0xFFFFFFFF)
    return dict(wave=(hw & np.uint64(15)).astype(int), simd=((hw >> np.uint64(4)) & np.uint64(3)).astype(int),
                cu=((hw >> np.uint64(8)) & np.uint64(15)).astype(int), se=((hw >> np.uint64(13)) & np.uint64(7)).astype(int),
                xcc=((x >> np.uint64(32)) & np.uint64(15)).astype(int), slot=((x >> np.uint64(40)) & np.uint64(255)).astype(int),
                wv=((x >> np.uint64(48)) & np.uint64(255)).astype(int), cuse=((hw >> np.uint64(8)) & np.uint64(255)).astype(int))
ti, pi = ids(st[:, 0, 13]), ids(st[:, 1, 13])
print("clips", len(tb), "T busy mean", tb.mean(), "P busy mean", pb.mean())
# Do waves w, w + 4, w + 8 of a workgroup share a SIMD, and no others? (chain2q_roles.hpp rests on it.) Asked of the two
# waves of every clip, which belong to one workgroup; the SIMD's number itself need not be w % 4
same = ti["simd"] == pi["simd"]
print("clips whose two waves share a SIMD exactly when their indices agree mod 4:", int((same == (ti["wv"] % 4 == pi["wv"] % 4)).sum()), "of", len(tb),
      "| SIMD == wave % 4: T", int((ti["simd"] == ti["wv"] % 4).sum()), "P", int((pi["simd"] == pi["wv"] % 4).sum()))
print("slot -> (T wave, P wave):", {int(s): (sorted(set(ti["wv"][ti["slot"] == s].tolist())), sorted(set(pi["wv"][pi["slot"] == s].tolist())))
                                   for s in np.unique(ti["slot"])})
# when the clips' bytes were out (record [14] of the packer, 100 MHz), as fractions of the launch: third argument = the
# launch's length in ms (the bench line's kernel_ms of the same run); the launch is taken to end with its last clip
if len(sys.argv) > 3:
    end = st[:, 1, 14].astype(np.float64) / 100.0    # us
    launch = float(sys.argv[3]) * 1e3
    frac = 1.0 - (end.max() - end) / launch
    print(f"clip end times / launch ({launch:.0f} us): first {frac.min():.4f} median {np.median(frac):.4f} last 1.0000 | "
          f"last - median {100 * (1 - np.median(frac)):.2f} % | deciles", np.round(np.quantile(frac, np.linspace(0, 1, 11)), 4).tolist())
    print("  by slot: (median, last)", {int(s): (round(float(np.median(frac[pi['slot'] == s])), 4), round(float(frac[pi['slot'] == s].max()), 4))
                                         for s in np.unique(pi["slot"])})
    print("  by T simd: (median, last)", {int(s): (round(float(np.median(frac[ti['simd'] == s])), 4), round(float(frac[ti['simd'] == s].max()), 4))
                                           for s in np.unique(ti["simd"])})
    # the last clip of every workgroup (CU): how far the CUs' ends are apart, against how far a CU's slots are
    cu_key = ti["xcc"] * 256 + ti["cuse"]
    cu_last = np.array([frac[cu_key == k].max() for k in np.unique(cu_key)])
    cu_first = np.array([frac[cu_key == k].min() for k in np.unique(cu_key)])
    print(f"  per CU ({len(cu_last)}): last slot's end min {cu_last.min():.4f} median {np.median(cu_last):.4f} max {cu_last.max():.4f}; "
          f"mean gap first-to-last slot inside a CU {100 * (cu_last - cu_first).mean():.2f} % of the launch")
for key in ("simd", "slot", "xcc", "se", "wave"):
    print("T by", key, {int(k): (round(float(tb[ti[key] == k].mean())), int((ti[key] == k).sum())) for k in np.unique(ti[key])})
for key in ("simd", "slot", "xcc"):
    print("P by", key, {int(k): (round(float(pb[pi[key] == k].mean())), int((pi[key] == k).sum())) for k in np.unique(pi[key])})
slow = tb > 11000
print("slow T clips:", slow.mean(), "their P busy", pb[slow].mean(), "others' P busy", pb[~slow].mean())
print("slow T by (T simd, P simd):")
for a in range(4):
    print("  ", [f"{(slow & (ti['simd'] == a) & (pi['simd'] == b)).sum()}/{((ti['simd'] == a) & (pi['simd'] == b)).sum()}" for b in range(4)])
print("corr(T busy, P busy) =", np.corrcoef(tb, pb)[0, 1])
for i, nm in enumerate(["fold", "prefetch", "fft", "postrot", "bandstats", "mask", "quant", "wait-consumed", "handover"]):
    print(f"  T {nm:14s} fast clips {t[~slow, i].mean() / hops:8.0f}   slow clips {t[slow, i].mean() / hops:8.0f}")
