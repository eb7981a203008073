"""Spectral similarity at collection scale: FingerprintIndex.topk_self(k=10) and .pairs(0.99) over N random-plus-planted
fingerprints (N = 10^4 and 10^5 by default), wall time and the event-timed device time of each call; the share of ordered
pairs whose exact score the bound filter skipped (the lane walk of the top-k kernel emulated on the host for sampled rows,
with the chunk length the library picks); and a chunked NumPy restatement of the score on the host for sampled rows, as
a rate to compare with. usage: python diag/similarity_time.py [N ...]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import flo_amd  # noqa: E402

F32 = np.float32
TERM = (F32(1.0) - np.arange(256, dtype=np.float32) / F32(255.0)).astype(np.float32)


def fingerprints(n, seed=1):
    """clustered random fingerprints (two formats) with planted duplicates: equal hashes, equal bytes"""
    rng = np.random.default_rng(seed)
    f = np.zeros(n, flo_amd.FINGERPRINT_DTYPE)
    f["hash"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    f["hash"][:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    f["sample_rate"] = np.where(rng.random(n) < 0.8, 44100, 48000)
    f["channels"] = 2
    centres = max(n // 250, 4)
    pick = rng.integers(0, centres, n)
    for fld, w in (("energy_profile", 16), ("frequency_peaks", 8)):
        c = rng.integers(0, 256, (centres, w))
        f[fld] = np.clip(c[pick] + rng.integers(-6, 7, (n, w)), 0, 255)
    f["avg_loudness"] = np.clip(rng.integers(40, 90, centres)[pick] + rng.integers(-3, 4, n), 0, 255)
    dup = rng.integers(0, n, (n // 100, 2))
    f["hash"][dup[:, 0]] = f["hash"][dup[:, 1]]
    same = rng.integers(0, n, (n // 100, 2))
    for fld in ("energy_profile", "frequency_peaks", "avg_loudness"):
        f[fld][same[:, 0]] = f[fld][same[:, 1]]
    return f


def host_scores(q, r):
    """the reference's f32 score of one query against every member (sequential sums, explicit f32 steps)"""
    e = np.zeros(len(r), np.float32)
    for k in range(16):
        e = (e + TERM[np.abs(r["energy_profile"][:, k].astype(np.int32) - int(q["energy_profile"][k]))]).astype(np.float32)
    p = np.zeros(len(r), np.float32)
    for k in range(8):
        p = (p + TERM[np.abs(r["frequency_peaks"][:, k].astype(np.int32) - int(q["frequency_peaks"][k]))]).astype(np.float32)
    lo = TERM[np.abs(r["avg_loudness"].astype(np.int32) - int(q["avg_loudness"]))]
    s = (((e / F32(16)) * F32(0.5)).astype(np.float32) + ((p / F32(8)) * F32(0.3)).astype(np.float32)).astype(np.float32)
    s = (s + (lo * F32(0.2)).astype(np.float32)).astype(np.float32)
    s = np.where((r["sample_rate"] == q["sample_rate"]) & (r["channels"] == q["channels"]), s, F32(0)).astype(np.float32)
    return np.where(np.all(r["hash"] == q["hash"], axis=1), F32(1), s).astype(np.float32)


def host_bounds(q, r):
    key = (5 * np.abs(r["energy_profile"].astype(np.int64) - q["energy_profile"]).sum(1)
           + 6 * np.abs(r["frequency_peaks"].astype(np.int64) - q["frequency_peaks"]).sum(1)
           + 32 * np.abs(r["avg_loudness"].astype(np.int64) - int(q["avg_loudness"])))
    u = ((F32(1) - (key.astype(np.float32) * (F32(1) / F32(40800))).astype(np.float32)) + F32(2.0 ** -17)).astype(np.float32)
    u = np.where((r["sample_rate"] == q["sample_rate"]) & (r["channels"] == q["channels"]), u, F32(0))
    return np.where(np.all(r["hash"] == q["hash"], axis=1), F32(1), u).astype(np.float32)


def exact_fraction(f, rows, k, chunk):
    """share of a row's candidates the top-k lane walk scores exactly: U >= its k-th score, chunk by chunk"""
    done = total = 0
    for i in rows:
        u, s = host_bounds(f[i], f), host_scores(f[i], f)
        for c0 in range(0, len(f), chunk):
            lst = []   # (score, index), best first
            for j in range(c0, min(len(f), c0 + chunk)):
                if j == i:
                    continue
                total += 1
                thr = lst[k - 1][0] if len(lst) >= k else -1.0
                if u[j] < thr:
                    continue
                done += 1
                if s[j] > thr:
                    lst.append((float(s[j]), j))
                    lst.sort(key=lambda x: (-x[0], x[1]))
                    del lst[k:]
    return done / max(total, 1)


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [10_000, 100_000]
    ctx = flo_amd.Context(0)
    name, cus, _ = ctx.device_info()
    print(f"device: {name} ({cus} CUs)")
    for n in sizes:
        f = fingerprints(n)
        ix = flo_amd.FingerprintIndex(f, ctx)
        ix.topk_self(10)
        ix.pairs(0.99)   # warm: code objects, pool blocks
        res = {}
        for what, fn, kern in (("topk_self(k=10)", lambda: ix.topk_self(10), ("fp_topk",)),
                               ("pairs(0.99)", lambda: ix.pairs(0.99), ("fp_pairs_count", "fp_pairs_write"))):
            walls, devs = [], []
            for _ in range(3):
                ctx.profile_enable(True)
                ctx.profile_reset()
                t = time.perf_counter()
                out = fn()
                walls.append(time.perf_counter() - t)
                devs.append(sum(ctx.profile_query(x)[0] for x in kern))
                ctx.profile_enable(False)
            res[what] = out
            print(f"N={n:>7}  {what:16s} wall {min(walls) * 1e3:9.2f} ms   device {min(devs):9.2f} ms   "
                  f"{n * (n - 1) / (min(devs) / 1e3) / 1e9:8.1f} G ordered pairs/s (device)")
        print(f"N={n:>7}  pairs(0.99) found {len(res['pairs(0.99)'][0])} pairs")
        # host restatement, sampled rows
        rng = np.random.default_rng(2)
        rows = rng.choice(n, 8, replace=False)
        t = time.perf_counter()
        for i in rows:
            host_scores(f[i], f)
        dt = time.perf_counter() - t
        print(f"N={n:>7}  host NumPy restatement: {len(rows) * n / dt / 1e6:.2f} M pairs/s (one core) -> "
              f"{n * (n - 1) / (len(rows) * n / dt):.0f} s for all ordered pairs")
        # the filter: the chunk length the library picks for a self-join of n rows (similarity.cpp: choose_chunk)
        tiles = -(-n // 256)
        want = max(1, -(-4 * cus // tiles))
        chunk = max(256, -(-(-(-n // want)) // 256) * 256)
        frac = exact_fraction(f, rows[:3], 10, chunk)
        print(f"N={n:>7}  top-k filter (chunk {chunk}): exact scores for {frac * 100:.3f} % of the pairs, "
              f"{(1 - frac) * 100:.3f} % rejected by the bound")
        # the pairs walk: U >= 0.99
        kept = np.mean([np.mean(host_bounds(f[i], f) >= F32(0.99)) for i in rows])
        print(f"N={n:>7}  pairs filter: exact scores for {kept * 100:.4f} % of the pairs")
        ix.close()
    ctx.close()


if __name__ == "__main__":
    main()
