"""The lossless encoder's rarely taken paths on the device: every case of ll_model.cases() through the C ABI.

The cases are built so that ll_model (pinned to the oracle by tests/test_ll_model_cpu.py) says which path of ll_prepare,
ll_analyze and ll_pack each one takes: both bit writers, tiles around the staging limit, long and capped codes, the third
sweep from both sides, ties, Levinson's early returns, the residual discard, short planes, every byte alignment of the
residual stream. For each case
  - ctx.encode_lossless equals the oracle's bytes; a mismatch names the first differing frame, channel and field and the
    paths the model predicts for the case,
  - the oracle's decode of the DEVICE file equals the model's integers, except for the reference's own undecodable quirk (a
    Raw-typed frame that holds Rice bytes, or a raw winner on a mid plane beyond 16 bits), decided by ll_model.undecodable
    from the model alone; those cases are counted (ll_model.EXPECTED_UNDECODABLE) and none of them is a packer case,
  - the device's decode of that file equals the oracle's decode of it (the parallel decoder on dense streams too).
Then the cases run side by side: one ragged encode_batch per (sr, ch, level), Batch.pack_files, and the streaming encoder.
All comparisons are exact. Needs an MI355X."""
import numpy as np
import pytest

import flofile
import ll_model as M
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CASES = M.cases()
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def ref():
    """name -> (model frames, oracle bytes), computed once and left unchanged"""
    return {c["name"]: (M.file_model(c["pcm"], c["sr"], c["ch"], c["level"]),
                        O.encode_lossless(c["pcm"], c["sr"], c["ch"], 16, c["level"])) for c in CASES}


def first_difference(g, o):
    """(frame, channel, field) of the first place two lossless files differ, like _same of test_gpu_lossless.py"""
    if len(g) < 70 or g[:4] != b"FLO!":
        return "not a file"
    try:
        fg, fo = flofile.parse(g), flofile.parse(o)
    except Exception as e:          # the container itself is broken
        return f"unparsable: {e!r}"
    for i, (a, b) in enumerate(zip(fg.frames, fo.frames)):
        for field in ("frame_type", "frame_samples", "flags", "size"):
            if getattr(a, field) != getattr(b, field):
                return (i, None, field, getattr(a, field), getattr(b, field))
        for c, (x, y) in enumerate(zip(a.channels, b.channels)):
            for field in ("coeffs", "shift_bits", "encoding", "rice_k"):
                if getattr(x, field) != getattr(y, field):
                    return (i, c, field, getattr(x, field), getattr(y, field))
            if len(x.residuals) != len(y.residuals):
                return (i, c, "payload length", len(x.residuals), len(y.residuals))
            if x.residuals != y.residuals:
                at = next(j for j, (p, q) in enumerate(zip(x.residuals, y.residuals)) if p != q)
                return (i, c, "payload byte", at, x.residuals[at], y.residuals[at])
    return "header, TOC or CRC" if len(fg.frames) == len(fo.frames) else ("frame count", len(fg.frames), len(fo.frames))


def assert_same(g, o, name, frames, how):
    if g != o:
        c = BY_NAME[name]
        tiles = [[(t["t0"], t["bits"], t["lead"], "staged" if t["staged"] else "UNSTAGED") for t in cm.tiles if not t["staged"] or t["long_code"]][:6]
                 for fm in frames if not fm.silent for cm in fm.channels]
        raise AssertionError(f"{name} via {how}: device file differs from the oracle at {first_difference(g, o)}; "
                             f"model paths {sorted(M.paths(frames, c['level']))}; unstaged / long-code tiles {tiles}")


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_case_file_and_decodes(ctx, ref, name):
    c = BY_NAME[name]
    frames, o = ref[name]
    g = ctx.encode_lossless(c["pcm"], c["sr"], c["ch"], 16, c["level"])
    assert_same(g, o, name, frames, "encode_lossless")
    back, sr, ch = O.decode_lossless_i32(g)
    assert (sr, ch) == (c["sr"], c["ch"])
    if not M.undecodable(frames):
        want = M.expected_ints(frames, c["ch"])
        assert back.size == want.size and np.array_equal(back, want), (name, int(np.argmax(back != want)) if back.size == want.size else (back.size, want.size))
    dev = ctx.decode_lossless_i32(g)
    assert dev.size == back.size and np.array_equal(dev, back), name


def test_exemptions_are_counted_and_no_packer_case_is_exempt(ref):
    ex = [n for n, (frames, _) in ref.items() if M.undecodable(frames)]
    assert len(ex) == M.EXPECTED_UNDECODABLE, ex
    assert 10 * len(ex) < len(CASES)
    assert not [n for n in ex if BY_NAME[n]["group"] == "packer"]


def _groups():
    g = {}
    for c in CASES:
        g.setdefault((c["sr"], c["ch"], c["level"]), []).append(c["name"])
    return g


def test_ragged_batches_per_group(ctx, ref):
    import flo_amd
    for (sr, ch, level), names in _groups().items():
        outs = ctx.encode_batch(flo_amd.MODE_LOSSLESS, [BY_NAME[n]["pcm"] for n in names], sr, ch, level)
        for n, g in zip(names, outs):
            assert_same(g, ref[n][1], n, ref[n][0], f"encode_batch of {len(names)} at {(sr, ch, level)}")


def test_packed_files_per_group(ctx, ref):
    import torch
    import flo_amd
    for (sr, ch, level), names in _groups().items():
        clips = [BY_NAME[n]["pcm"] for n in names]
        b = flo_amd.Batch(ctx, flo_amd.MODE_LOSSLESS, [c.size for c in clips], sr, ch, level)
        for i, c in enumerate(clips):
            if c.size:
                b.upload(i, c)
        b.encode(0)
        b.sync()
        buf = torch.empty(b.data_bytes() + len(clips) * 256 + 1024, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        offs = b.pack_files(buf.data_ptr(), buf.numel())
        b.sync()
        host = buf.cpu().numpy()
        for i, n in enumerate(names):
            want = ref[n][1]
            assert_same(host[offs[i]:offs[i] + len(want)].tobytes(), want, n, ref[n][0], f"pack_files at {(sr, ch, level)}")
        b.close()


@pytest.mark.parametrize("name", ["dense96_middle_l5", "sweep3_winner_l5"])
def test_streaming_encoder_takes_the_same_paths(ctx, name):
    import flo_amd
    c = BY_NAME[name]
    g = flo_amd.StreamingEncoder(c["sr"], c["ch"], 16, ctx).with_compression(c["level"])
    o = O.StreamingEncoder(c["sr"], c["ch"], 16, c["level"])
    half = (c["pcm"].size // 2 // c["ch"]) * c["ch"]
    for part in (c["pcm"][:half], c["pcm"][half:]):
        g.push_samples(part)
        o.push_samples(part)
    fg, fo = g.finalize(), o.finalize()
    g.close()
    assert_same(fg, fo, name, M.file_model(c["pcm"], c["sr"], c["ch"], c["level"]), "StreamingEncoder")
