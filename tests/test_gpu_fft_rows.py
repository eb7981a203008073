"""The FFT of the stereo chain encode (lossy_chain2q_kernel, form 5) with its twiddle rows resident in registers
(fft512_2_tw: rows kRowF1 / kRowF2 loaded once per launch) and the half-frame prefetch issued behind the FFT instead of at
the top of the frame. Forms 1 (one wave per channel) and 2 (frame-parallel: fft512_2 and fold_2, which read every row from
the pack every frame and load both halves up front) are the independent yardsticks: every file of form 5 equals the same
clip's file under both, byte for byte, and the coefficients form 5 hands out (LossyArgs::dbg_coeffs, through
ctx.lossy_analyze) are forms 1's and 2's bit for bit and within the suite's coefficient bound of the oracle's (1e-5
relative RMS, gpu_util.compare_lossy_stage).

Clips are stereo, q = 0.55. A clip of n sample-frames has ceil((n + 1024) / 1024) frames; behind its last frame the
kernel prefetches the spare half-frame the batch pads every clip with.

    frame counts    0, 300, 1024, 1500 and 2048 sample-frames: one frame that is only the pre-roll's carry, a clip shorter
                    than one frame (its second frame folds 300 samples and padding), exactly two frames, three frames ragged
                    and exact. The prefetch behind the only frame's FFT is the spare half-frame's
    clip change     1600 three-frame clips in one launch: more clips than (transform, packer) pairs on the device, so pairs
                    take a second clip: the resident rows and the prefetch must survive the change. Eight different
                    clips in turn, so neighbours on a slot differ
    ragged          clips of 1, 2, 5 and 17 frames mixed, at six slots per workgroup
    silence         all-zero clips of 1, 2 and 3 frames
    sine            a full-scale sine (amplitude 1.0, the other channel in antiphase at another frequency) at 44.1 and 48 kHz
Needs an MI355X."""
import numpy as np
import pytest

import flo_amd  # noqa: F401
import signals
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O
from test_gpu_fold_carry import check, frames
from test_gpu_lossy_paths import forced

pytestmark = pytest.mark.gpu
CH, Q = 2, 0.55
COEF_REL_RMS = 1e-5       # gpu_util.compare_lossy_stage's bound on the coefficients


def coefficients_agree(ctx, pcm, sr, tag):
    """form 5's dbg_coeffs against forms 1 and 2 (bit for bit) and against the oracle (relative RMS)"""
    got = {}
    for form in (5, 1, 2):
        with forced(ctx, form):
            got[form] = ctx.lossy_analyze(pcm, sr, CH, Q)["coeffs"]
    co = O.lossy_analyze(pcm, sr, CH, Q)["coeffs"].astype(np.float64)
    assert got[5].shape == co.shape
    den = (co ** 2).sum()
    rel = float(np.sqrt(((got[5].astype(np.float64) - co) ** 2).sum() / den)) if den > 0 else float(np.abs(got[5]).max())
    print(f"{tag}: coefficient relative RMS against the oracle {rel:.3e}")
    assert rel <= COEF_REL_RMS, (tag, "coefficient relative RMS", rel)
    for form in (1, 2):
        bad = np.argwhere(got[5].view(np.uint32) != got[form].view(np.uint32))
        assert bad.size == 0, (tag, "coefficients of form 5 and form", form, "first (frame, channel, position)", bad[0].tolist(),
                               float(got[5][tuple(bad[0])]), float(got[form][tuple(bad[0])]))


FRAME_LENS = [0, 300, 1024, 1500, 2048]


@pytest.mark.parametrize("sr", [44100, 48000])
def test_clips_of_one_two_and_three_frames_and_shorter_than_a_frame(ctx, sr):
    assert [frames(n) for n in FRAME_LENS] == [1, 2, 2, 3, 3]
    clips = [signals.music_like(sr, n, CH, seed=410 + i) for i, n in enumerate(FRAME_LENS)]
    check(ctx, clips, sr, "1, 2 and 3 frames")
    # (the 0-sample clip too: its only frame is the pre-roll's carry folded with the spare half-frame, every coefficient zero)
    for n, pcm in zip(FRAME_LENS, clips):
        coefficients_agree(ctx, pcm, sr, f"{n} sample-frames at {sr} Hz")


def test_pairs_take_a_second_clip(ctx):
    sr, n = 44100, 1500
    assert frames(n) == 3
    pairs = int(ctx.device_info()[1]) * 6
    assert pairs < 1600, ("every pair of the device takes one clip at the most", pairs)
    base = [signals.music_like(sr, n, CH, seed=420 + i) if i & 1 else signals.fast_noise(2 * n, seed=420 + i, amp=0.9) for i in range(8)]
    check(ctx, [base[i % 8] for i in range(1600)], sr, "1600 clips of three frames")


def test_ragged_batch_of_1_2_5_and_17_frames(ctx):
    sr = 44100
    lens = [16000, 0, 700, 3500, 0, 16000, 3500, 700, 700, 0, 16000, 3500, 0]
    assert sorted({frames(n) for n in lens}) == [1, 2, 5, 17]
    clips = [signals.music_like(sr, n, CH, seed=430 + i) for i, n in enumerate(lens)]
    check(ctx, clips, sr, "ragged", override=6)
    check(ctx, clips, sr, "ragged, one slot per workgroup", override=1, refs=(1,))


def test_silence(ctx):
    sr = 44100
    clips = [np.zeros(2 * n, np.float32) for n in (0, 700, 2048)]
    got = check(ctx, clips, sr, "silence")
    with forced(ctx, 5):
        g = ctx.lossy_analyze(clips[2], sr, CH, Q)
    assert not g["coeffs"].any() and not g["q"].any()
    assert len(got[2]) > 0


@pytest.mark.parametrize("sr", [44100, 48000])
def test_full_scale_sine(ctx, sr):
    n = 2900
    assert frames(n) == 4
    x = np.empty((n, 2), np.float32)
    x[:, 0] = signals.sine(997.0, sr, n, amp=1.0)
    x[:, 1] = -signals.sine(5512.5, sr, n, amp=1.0)
    assert np.abs(x).max() > 0.999
    pcm = x.reshape(-1)
    check(ctx, [pcm], sr, "full-scale sine")
    coefficients_agree(ctx, pcm, sr, f"full-scale sine at {sr} Hz")
