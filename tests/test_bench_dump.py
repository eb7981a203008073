"""bench.py --dump-outputs: what the timed path computed in its last step, written so two builds can be compared."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bench
import flofile
from gpu_util import ctx  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("file_bytes", "file_crc32", "sample_clips", "sample_files")


def _load(d):
    out = {k: np.load(os.path.join(d, k + ".npy")) for k in NAMES}
    for k, a in out.items():
        assert a.dtype in (np.float32, np.float64), (k, a.dtype)
    assert sum(os.path.getsize(os.path.join(d, k + ".npy")) for k in NAMES) <= bench.DUMP_LIMIT_BYTES <= 64_000_000
    return out


def _sampled(dump):
    """the sampled files cut back out of the concatenation, as bytes"""
    flat = dump["sample_files"]
    assert ((flat >= 0) & (flat <= 255) & (flat == np.floor(flat))).all()
    files, pos = [], 0
    for i in dump["sample_clips"].astype(np.int64):
        n = int(dump["file_bytes"][i])
        files.append(flat[pos:pos + n].astype(np.uint8).tobytes())
        pos += n
    return files, pos


class _FakeBatch:
    def __init__(self, sizes):
        self.n_clips = len(sizes)
        self._files = [np.random.default_rng(i).integers(0, 256, n, dtype=np.uint8).tobytes() for i, n in enumerate(sizes)]

    def fetch(self, clip):
        return self._files[clip]


def test_dump_keeps_whole_files_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 24 * 40 + 4 * 5000)   # room for 5000 sampled bytes
    b = _FakeBatch([700 + 37 * i for i in range(40)])
    bench.dump_outputs(b, str(tmp_path / "a"))
    bench.dump_outputs(b, str(tmp_path / "b"))
    a, again = _load(tmp_path / "a"), _load(tmp_path / "b")
    for k in NAMES:
        assert np.array_equal(a[k], again[k]), k
    assert np.array_equal(a["file_bytes"], [len(f) for f in b._files])
    assert np.array_equal(a["file_crc32"], [zlib.crc32(f) for f in b._files])
    files, used = _sampled(a)
    assert 1 <= len(files) < 40 and used == a["sample_files"].size <= 5000
    assert len(set(a["sample_clips"].tolist())) == len(files)
    assert all(f == b._files[int(i)] for f, i in zip(files, a["sample_clips"]))


def test_dump_cuts_a_file_larger_than_the_limit_to_its_head(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 24 * 2 + 4 * 1000)
    b = _FakeBatch([3000, 2500])
    bench.dump_outputs(b, str(tmp_path))
    d = _load(tmp_path)
    i = int(d["sample_clips"][0])
    assert d["sample_clips"].size == 1 and d["sample_files"].size == 1000
    assert d["sample_files"].astype(np.uint8).tobytes() == b._files[i][:1000]


@pytest.mark.gpu
def test_bench_dumps_the_files_of_its_last_step(tmp_path, ctx):
    # two runs with different step counts over the same seeded inputs write the same outputs, and they are the files a
    # caller of the benchmarked path gets from an encode of the same clips (256 stereo clips: the lock-step chain form)
    import flo_amd
    n, sr, ch = 256, 44100, 2
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--clips-per-gpu", str(n), "--clip-seconds", "2",
            "--no-cpu-baseline", "--no-single-clip", "--no-lossless", "--no-shard", "--no-e2e"]
    dumps = []
    for tag, steps, warmup in (("a", "1", "0"), ("b", "3", "1")):
        r = subprocess.run(base + ["--steps", steps, "--warmup", warmup, "--dump-outputs", str(tmp_path / tag)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith('{"metric"')][-1])
        assert line["steps"] == int(steps) and line["value"] > 0
        dumps.append(_load(tmp_path / tag))
    for k in NAMES:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
    d = dumps[0]
    files, _ = _sampled(d)
    assert len(files) == n        # files of two seconds all fit whole
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [2 * sr * ch] * n, sr, ch, 0.55)
    b.fill_synthetic(seed=0xF10A0D10, clip_id0=0)
    b.encode(0)
    b.sync()
    mine = [b.fetch(i) for i in range(n)]
    b.close()
    assert np.array_equal(d["file_bytes"], [len(f) for f in mine])
    assert np.array_equal(d["file_crc32"], [zlib.crc32(f) for f in mine])
    for f, i in zip(files, d["sample_clips"].astype(np.int64)):
        assert f == mine[i] and flofile.parse(f).crc_valid
