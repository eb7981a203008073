"""The model of the partitioned FFT convolution (tests/fftconv_model.py) against the exact f64 convolution, on the CPU: on
the shapes its docstring quotes for B = 256, 512 and 1024, and on every job of the device cases of tests/test_gpu_fftconv.py
at the geometry in force. Every figure stays under R_CAP = 2^-22, so a sloppy model cannot loosen the device's bound
(max(3 r_model, floor)); the figures measured here, 1.1e-8 to 6.0e-8 on the quoted shapes and up to 6.7e-8 on the device
cases, sit 3.5x inside it. Blocks of zero scale are zero."""
import numpy as np
import pytest

import fftconv_model as M

CASES = [(1, 1), (2, 1), (2, 2), (3, 1), (3, 3), (8, 1), (8, 8)]


@pytest.mark.parametrize("B", [256, 512, 1024])
def test_the_model_on_the_quoted_shapes(B):
    for name in M.CPU_SHAPES:
        x, h, g = M.cpu_shape(name, B)
        r, zero_ok = M.job_ratio(M.model_clip(x, 1, h, 1, g, B), x, 1, h, 1, g, B)
        print("B %d, %s: r %.2e" % (B, name, r))
        assert r <= M.R_CAP and zero_ok, (B, name, r)


def test_the_model_equals_the_direct_definition_where_it_is_exact():
    """a unit tap moves the source: the model's output is the shifted clip to within its own yardstick, and K == 0, N == 0
    and T == 0 give zeros of the right length"""
    B = 256
    x = M.noise(700, 2, 5)
    for d in (0, 1, B - 1, B, 2 * B):
        h = M.impulse(d + 1, 1, d)
        g = M.job(0, 0, 900)
        y = M.model_clip(x, 2, h, 1, g, B).reshape(900, 2)
        want = np.zeros((900, 2))
        want[d:d + 700] = x.reshape(700, 2)[:900 - d]
        assert np.abs(y - want).max() <= 2.0 ** -22 * np.sqrt(2 * B) * 0.3 * 4, d
    assert not M.model_clip(x, 2, np.zeros(0, M.F32), 1, M.job(0, 0, 50), B).any()
    assert M.model_clip(x, 2, np.ones(3, M.F32), 1, M.job(0, 0, 0), B).size == 0
    assert not M.model_clip(np.zeros(0, M.F32), 2, np.ones(3, M.F32), 1, M.job(0, 0, 40), B).any()


@pytest.mark.parametrize("ch,ir_ch", CASES)
def test_the_model_on_the_device_cases(ch, ir_ch):
    import flo_amd
    geo = flo_amd.conv_fft_geometry(ch, ir_ch)
    B, LB = geo["block_frames"], geo["lane_blocks"]
    src, irs, jobs = M.device_case(ch, ir_ch, B, LB, sweeps=(ch, ir_ch) in ((1, 1), (2, 2)), big=(ch, ir_ch) == (2, 1))
    assert max(x.size // ch for x in src[:6]) <= 3 * LB * B + 5
    worst = 0.0
    for k, g in enumerate(jobs):
        x, h = src[g["clip"]], irs[g["ir"]]
        r, zero_ok = M.job_ratio(M.model_clip(x, ch, h, ir_ch, g, B), x, ch, h, ir_ch, g, B)
        assert r <= M.R_CAP and zero_ok, (k, g, r)
        worst = max(worst, r)
    print("C %d, Ch %d: %d jobs, largest r_model %.2e" % (ch, ir_ch, len(jobs), worst))


def test_segments_and_reach():
    B = 256
    assert M.stored_segments(0, 100, 5, 0, B) == 0 and M.stored_segments(100, 100, 0, 0, B) == 0
    assert M.stored_segments(1, 1, 1, 0, B) == 1                       # segment 0 alone: segment 1 has no block
    assert M.stored_segments(3 * B, 4 * B, B, 0, B) == 4               # q = 0 .. 3
    assert M.stored_segments(3 * B, 4 * B, B, B, B) == 3               # skip B: q = 0 .. 2 (q = -1 is no block's: Pn = 1)
    assert M.stored_segments(3 * B, 4 * B, B + 1, B, B) == 4           # Pn = 2: q = -1 .. 2
    assert M.reached_blocks(0, 0, 3 * B, B, B, 4) == [0, 1] and M.reached_blocks(B, 0, 3 * B, B + 1, B, 6) == [1, 2, 3]
