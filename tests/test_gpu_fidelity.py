"""Fidelity reports on the device (flo_batch_fidelity, flo_compare, `cli compare`) against the NumPy model of the documented
order (tests/fidelity_ref.py), bit for bit: lossy batches in the fused decode-and-compare pass and in the unfused one,
lossless batches, single files, the reference's example files, the oracle's decoder, errors and the CLI."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fidelity_ref as M
import flofile
import signals
from conftest import EXAMPLES, ROOT
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O

import flo_amd

pytestmark = pytest.mark.gpu

SR = 44100
LENGTHS = [1, 1023, 1024, 1025, int(12.3 * SR)]


def _decoded(b, rep):
    """every clip's decoded PCM (Batch.decode_to into device memory, then to the host); rep sizes it"""
    import torch
    total = sum(r["decoded_frames"] for r in rep) * b.channels
    out = torch.empty(max(total, 1), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    offs = b.decode_to(out.data_ptr(), out.numel())
    host = out.cpu().numpy()
    ends = offs[1:] + [total]
    return [host[offs[i]:ends[i]] for i in range(b.n_clips)]


def _batch(ctx, mode, clips, ch, q, bit_depth=None):
    b = flo_amd.Batch(ctx, mode, [c.size for c in clips], SR, ch, q)
    for i, c in enumerate(clips):
        b.upload(i, c)
    if bit_depth:
        b.set_bit_depth(bit_depth)
    b.encode(0)
    b.sync()
    return b


def _clips(ch, seed):
    out = []
    for k, n in enumerate(LENGTHS):
        x = signals.music_like(SR, n, ch, seed=seed + k).astype(np.float32).reshape(-1)
        if ch > 1 and k % 2:
            x = np.concatenate([x, np.float32([0.25] * (k % ch or 1))])   # n_interleaved % ch != 0
        out.append(x)
    return out


def _check_batch(b, tag):
    rep = b.fidelity(blocks=True)
    dec = _decoded(b, rep)
    for i in range(b.n_clips):
        want, wb = M.fidelity(b.download_pcm(i), dec[i], b.channels)
        M.assert_matches(rep[i], want, wb, tag=(tag, i))
    return rep


def _raw(rep):
    return b"".join(r["blocks"].tobytes() + b"".join(np.asarray(r[k]).tobytes() for k in sorted(r) if k != "blocks") for r in rep)


@pytest.mark.parametrize("ch", [1, 2, 6])
@pytest.mark.parametrize("q", [0.2, 0.55, 1.0])
def test_lossy_batch_matches_the_model_fused_and_unfused(ctx, ch, q, monkeypatch):
    b = _batch(ctx, flo_amd.MODE_LOSSY, _clips(ch, 100 * ch), ch, q)
    try:
        fused = _check_batch(b, ("fused", ch, q))
        again = b.fidelity(blocks=True)
        assert _raw(again) == _raw(fused)                           # two calls: identical bytes
        monkeypatch.setenv("FLO_FIDELITY_UNFUSED", "1")
        unfused = b.fidelity(blocks=True)
        assert _raw(unfused) == _raw(fused)                         # the unfused pass: identical bytes
        monkeypatch.delenv("FLO_FIDELITY_UNFUSED")
        r = fused[-1]
        assert r["decoded_frames"] - r["compared_frames"] < 1024 and r["compared_frames"] == r["source_frames"]
        assert np.all(np.isfinite(r["snr_db"])) and np.all(r["snr_db"] > 0)
        without = b.fidelity()
        assert "blocks" not in without[0] and _raw([dict(x, blocks=np.zeros(0)) for x in without]) == \
            _raw([dict(x, blocks=np.zeros(0)) for x in fused])
    finally:
        b.close()


@pytest.mark.parametrize("bits", [16, 24])
def test_lossless_batch_matches_the_model(ctx, bits):
    clips = _clips(2, 7 + bits)
    b = _batch(ctx, flo_amd.MODE_LOSSLESS, clips, 2, 5, bit_depth=bits)
    try:
        rep = _check_batch(b, ("lossless", bits))
        assert all(r["decoded_frames"] == r["source_frames"] for r in rep)
    finally:
        b.close()


def test_lossless_file_against_the_devices_own_decode_is_exact(ctx):
    clips = _clips(2, 3)
    b = _batch(ctx, flo_amd.MODE_LOSSLESS, clips, 2, 5)
    try:
        for i in range(b.n_clips):
            f = b.fetch(i)
            r = ctx.compare(ctx.decode(f), f, blocks=True)
            assert np.all(r["blocks"]["error"] == 0.0) and np.all(r["error"] == 0.0), i
            assert np.all(r["snr_db"] == np.inf) and r["snr_db_all"] == np.inf, i
            assert r["compared_frames"] == r["decoded_frames"] == r["source_frames"], i
    finally:
        b.close()


@pytest.mark.parametrize("mode", [flo_amd.MODE_LOSSY, flo_amd.MODE_LOSSLESS])
def test_compare_of_a_fetched_file_equals_the_batch_report(ctx, mode):
    clips = _clips(2, 50)
    b = _batch(ctx, mode, clips, 2, 0.55 if mode == flo_amd.MODE_LOSSY else 5)
    try:
        rep = b.fidelity(blocks=True)
        for i in range(b.n_clips):
            got = ctx.compare(clips[i], b.fetch(i), blocks=True)
            assert _raw([got]) == _raw([rep[i]]), i
    finally:
        b.close()


def test_example_files_compare_to_their_own_decode_with_zero_error(ctx):
    names = sorted(n for n in os.listdir(EXAMPLES) if n.endswith(".flo"))
    assert len(names) >= 10
    for n in names:
        f = open(os.path.join(EXAMPLES, n), "rb").read()
        y = ctx.decode(f)
        r = ctx.compare(y, f, blocks=True)
        assert np.all(r["error"] == 0.0) and np.all(r["blocks"]["error"] == 0.0), n
        assert r["decoded_frames"] == r["compared_frames"], n
        assert np.all(r["tail_energy"] == 0.0), n


@pytest.mark.parametrize("q", [0.2, 0.35, 0.55])
def test_snr_agrees_with_the_oracle_decoder(ctx, q):
    pcm = signals.music_like(SR, 120000, 2, seed=17).astype(np.float32).reshape(-1)
    f = O.encode_lossy(pcm, SR, 2, q)
    r = ctx.compare(pcm, f)
    o, _, _ = O.decode(f)
    want, _ = M.fidelity(pcm, o, 2)
    assert np.all(np.abs(r["snr_db"] - want["snr_db"]) < 0.01), (r["snr_db"], want["snr_db"])
    assert abs(flo_amd.compare(pcm, f)["snr_db_all"] - r["snr_db_all"]) == 0.0


def test_errors(ctx):
    b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSY, [4096], SR, 1, 0.5)
    try:
        b.upload(0, np.zeros(4096, np.float32))
        with pytest.raises(flo_amd.FloError, match="sync"):
            b.fidelity()                                            # FLO_ERR_STATE before encode + sync
        b.encode(0)
        b.sync()
        L = ctx._L
        off = np.zeros(2, np.uint64)
        assert L.flo_batch_fidelity(b._h, None, None, 0, None) == 1                      # FLO_ERR_ARG
        out = np.zeros(1, flo_amd.FIDELITY_DTYPE)
        blk = np.zeros(1, flo_amd.FIDELITY_BLOCK_DTYPE)
        assert L.flo_batch_fidelity(b._h, out.ctypes.data, blk.ctypes.data, 1, off.ctypes.data) == 1   # 4 blocks, room for 1
        assert L.flo_batch_fidelity(b._h, None, None, 0, off.ctypes.data) == 0 and off[-1] == 4
    finally:
        b.close()
    pcm = signals.music_like(SR, 5000, 2, seed=1).astype(np.float32).reshape(-1)
    good = ctx.encode_lossy(pcm, SR, 2, 0.5)
    with pytest.raises(flo_amd.FloError):
        ctx.compare(pcm, b"not a flo file at all")                  # FLO_ERR_FORMAT
    L = ctx._L
    out = np.zeros(2, flo_amd.FIDELITY_DTYPE)
    assert L.flo_compare(ctx._h, pcm.ctypes.data, pcm.size, b"junk" * 40, 160, out.ctypes.data, None, 0, None) == 5
    assert L.flo_compare(ctx._h, pcm.ctypes.data, pcm.size, good, len(good), None, None, 0, None) == 1
    blk = np.zeros(2, flo_amd.FIDELITY_BLOCK_DTYPE)
    assert L.flo_compare(ctx._h, pcm.ctypes.data, pcm.size, good, len(good), out.ctypes.data, blk.ctypes.data, 2, None) == 1
    # a transform frame that does not deserialise: flo_decode's message
    bad = bytearray(good)
    bad[70 + flofile.parse(good).toc_size + 10 + 1] = 7              # the first blob claims more channels than the header
    with pytest.raises(flo_amd.FloError, match="deserialize"):
        ctx.decode(bytes(bad))
    with pytest.raises(flo_amd.FloError, match="deserialize"):
        ctx.compare(pcm, bytes(bad))


def test_profile_hooks_see_the_launches(ctx):
    b = _batch(ctx, flo_amd.MODE_LOSSY, _clips(2, 9)[:3], 2, 0.55)
    try:
        ctx.profile_enable(True)
        ctx.profile_reset()
        b.fidelity()
        ms, n = ctx.profile_query("fidelity")
        ctx.profile_enable(False)
        assert n == 2 and ms > 0.0                                  # the fused pass and the totals
    finally:
        b.close()


def test_cli_compare(ctx, tmp_path):
    from flo_amd.wav import read_wav_bytes, write_wav_bytes
    pcm = signals.music_like(SR, 70000, 2, seed=23).astype(np.float32).reshape(-1)
    wav = tmp_path / "src.wav"
    wav.write_bytes(write_wav_bytes(pcm, SR, 2))
    flo = tmp_path / "src.flo"
    flo.write_bytes(O.encode_lossy(pcm, SR, 2, 0.55))
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = [sys.executable, "-m", "flo_amd.cli", "compare", str(wav), str(flo)]
    src, _, _ = read_wav_bytes(wav.read_bytes())
    want, wb = M.fidelity(src, ctx.decode(flo.read_bytes()), 2)
    r = subprocess.run(run + ["--json", "--blocks"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout)
    assert rep["compared_frames"] == want["compared_frames"] and rep["decoded_frames"] == want["decoded_frames"]
    for k in range(2):
        p = rep["per_channel"][k]
        assert float(p["snr_db"]) == pytest.approx(want["snr_db"][k], abs=1e-9)
        assert float(p["seg_snr_db"]) == pytest.approx(want["seg_snr_db"][k], abs=1e-9)
        assert float(p["signal"]) == want["signal"][k] and float(p["error"]) == want["error"][k]
        assert float(p["tail_energy"]) == want["tail_energy"][k] and p["clipped"] == int(want["clipped"][k])
        assert float(p["peak_error"]) == float(want["peak_error"][k])
    assert len(rep["block_snr_db"]) == wb.shape[0]
    t = subprocess.run(run, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert t.returncode == 0, t.stderr
    assert f"SNR {want['snr_db'][0]:.4f} dB" in t.stdout and f"{want['compared_frames']} compared" in t.stdout
    # a WAV whose format does not match the file is refused
    wav48 = tmp_path / "w48.wav"
    wav48.write_bytes(write_wav_bytes(pcm, 48000, 2))
    m = subprocess.run([sys.executable, "-m", "flo_amd.cli", "compare", str(wav48), str(flo)], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert m.returncode == 1 and "48000" in m.stderr
