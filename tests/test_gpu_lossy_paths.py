"""The lossy encoder's hidden paths on the device, case by case (tests/lossy_model.py names the paths; its CPU test asserts
that every path has a case here).

    packer wave   hand-made spectra through flo_lossy_pack_frames under forms 5, 1 and 2: the device's integers equal the
                  oracle's, and the bytes equal lossy_model.write_frames applied to the device's own integers
    dealing       ragged batches under form 5 (by batch size and by FLO_CHAIN2X_CLIPS): every file equals the same clip
                  encoded alone under form 1
    geometry      form 2 (and auto) against form 1: scan blocks, compaction variants, offset scans, the hand-over's edge
    levels        clips whose masking level does not decay (a band energy that overflows f32): all forms and routes give the
                  sequential chain's bytes, and a blob is empty exactly where the oracle's integers are all zero
Every failure names the case, clip, frame, channel, the first differing byte and the model's paths of that frame.
"""
import os

import numpy as np
import pytest

import flo_amd
import flofile
import lossy_model as M
from gpu_util import ctx  # noqa: F401
from oracle import oracle as O

pytestmark = pytest.mark.gpu
SR = 44100


class forced:
    """force a kernel form and environment switches for the block, and put both back"""

    def __init__(self, ctx, which, **env):
        self.ctx, self.which, self.env, self.old = ctx, which, env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        self.ctx.force_path(self.which)

    def __exit__(self, *exc):
        self.ctx.force_path(0)
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return int(d[0]) if d.size else (n if len(a) != len(b) else None)


def describe_data_difference(tag, got, want, nch, paths=None):
    """the frame, channel and byte at which two DATA chunks part"""
    at = first_difference(got, want)
    if at is None:
        return None
    msg = f"{tag}: DATA differs at byte {at} (lengths {len(got)} / {len(want)})"
    try:
        p = 0
        for h, (f, blobs) in enumerate(M.split_frames(want, nch)):
            if at < p + len(f):
                o = at - p
                c = 12 + 50 * nch
                field = "header" if o < 12 else "scale words" if o < c else None
                for ch, b in enumerate(blobs):
                    if field is None and o < c + 4 + len(b):
                        field = f"channel {ch} " + ("length word" if o < c + 4 else f"blob byte {o - c - 4} of {len(b)}")
                    c += 4 + len(b)
                msg += f": frame {h}, offset {o}, {field}"
                if paths is not None:
                    msg += f"; paths {sorted(paths[h])}"
                break
            p += len(f)
    except AssertionError:
        msg += " (the expected DATA does not split into frames)"
    return msg


# ------------------------------------------------------------------------------------------------ packer wave
SPECTRA = M.spectra_cases() + [M.levels_spectra_case()] + M.spectra_cases_other_channels()
_oracle_q = {}


def oracle_q(name):
    if name not in _oracle_q:
        _, c, sr, q = next(x for x in SPECTRA if x[0] == name)
        _oracle_q[name] = O.lossy_quantize(c, sr, q)
    return _oracle_q[name]


@pytest.mark.parametrize("form", [5, 1, 2])
@pytest.mark.parametrize("name", [c[0] for c in SPECTRA])
def test_packer_wave_on_hand_made_spectra(ctx, name, form):
    _, c, sr, q = next(x for x in SPECTRA if x[0] == name)
    o = oracle_q(name)
    with forced(ctx, form):
        g = ctx.lossy_pack_frames(c, sr, q)
    bad = np.argwhere(g["q"] != o["q"])
    assert bad.size == 0, (name, form, "integers differ from the oracle's", len(bad), "first (frame, channel, position)", bad[0].tolist(),
                           int(g["q"][tuple(bad[0])]), int(o["q"][tuple(bad[0])]))
    assert np.array_equal(g["sf_words"], o["sf_words"]), (name, form, "scale words", np.argwhere(g["sf_words"] != o["sf_words"])[0].tolist())
    want, sizes = M.write_frames(g["q"], g["sf_words"])
    nch = c.shape[1]
    paths = M.frame_paths(g["q"], sizes, sr) if nch == 2 else None      # (the model names the stereo packer's paths)
    assert g["frame_sizes"].tolist() == sizes, (name, form, "frame sizes", g["frame_sizes"].tolist(), sizes)
    msg = describe_data_difference(f"{name} form {form}", g["data"], want, nch, paths)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------ dealing
_alone = {}


def alone_form1(ctx, pcm, ch, key):
    """the clip encoded alone under form 1 (kept per distinct clip: the batches repeat them)"""
    if key not in _alone:
        with forced(ctx, 1):
            _alone[key] = ctx.encode_lossy(pcm, SR, ch, 0.55)
    return _alone[key]


def ragged_batch(ch, lens):
    """clips that differ: content by i mod 97, length by the list (four music clips among tone bursts)"""
    keys = [(ch, n, i if i < 16 and i % 8 in (3, 5) else 16 + i % 97) for i, n in enumerate(lens)]
    made = {}
    for k in keys:
        if k not in made:
            made[k] = M.ragged_clip(k[1], ch, k[2])
    return [made[k] for k in keys], keys


def check_batch_against_alone(ctx, tag, ch, lens, which, env, kernel=None):
    clips, keys = ragged_batch(ch, lens)
    refs = [alone_form1(ctx, p, ch, k) for p, k in zip(clips, keys)]
    with forced(ctx, which, **env):
        if kernel:
            ctx.profile_enable(True)
            ctx.profile_reset()
        try:
            files = ctx.encode_batch(1, clips, SR, ch, 0.55)
            if kernel:
                ran = {k: ctx.profile_query(k)[1] for k in ("lossy_chain2q", "lossy_chain", "lossy_frames")}
                assert ran == {k: (1 if k == kernel else 0) for k in ran}, (tag, "kernels launched", ran)
        finally:
            if kernel:
                ctx.profile_enable(False)
    assert len(files) == len(refs)
    for i, (f, r) in enumerate(zip(files, refs)):
        if f != r:
            pf, pr = flofile.parse(f), flofile.parse(r)
            msg = describe_data_difference(f"{tag} clip {i} ({lens[i]} sample-frames)", pf.data, pr.data, ch)
            raise AssertionError(msg or f"{tag} clip {i}: header or TOC differs at byte {first_difference(f, r)}")


def n_cus(ctx):
    return int(ctx.device_info()[1])


DEALING = M.dealing_batches()


@pytest.mark.parametrize("index", [i for i, d in enumerate(DEALING) if d[3] == 5], ids=[d[0] for d in DEALING if d[3] == 5])
def test_dealing_form5_equals_each_clip_alone(ctx, index):
    cus = n_cus(ctx)
    name, ch, lens, which, g = M.dealing_batches(cus)[index]      # (the ragged batch is sized by the device's compute units)
    if name.startswith("ragged"):
        assert len(lens) > 6 * cus, "the batch must hold more clips than 6 x compute units"
        assert "deal:persistent" in M.batch_paths(ch, lens, 5, cus, g)
    check_batch_against_alone(ctx, name, ch, lens, which, {"FLO_CHAIN2X_CLIPS": g or None})


@pytest.mark.parametrize("name,kernel", [("auto_ch1_511", "lossy_frames"), ("auto_ch1_512", "lossy_chain"),
                                         ("auto_ch2_255", "lossy_frames"), ("auto_ch2_256", "lossy_chain2q")])
def test_auto_rule_picks_the_kernel_and_the_files_equal_each_clip_alone(ctx, name, kernel):
    _, ch, lens, which, _ = next(d for d in DEALING if d[0] == name)
    check_batch_against_alone(ctx, name, ch, lens, 0, {"FLO_CHAIN2X_CLIPS": None}, kernel)


# ------------------------------------------------------------------------------------------------ geometry
def forms_agree(ctx, tag, clips, ch, forms=(1, 2)):
    out = []
    for w in forms:
        with forced(ctx, w):
            out.append(ctx.encode_batch(1, clips, SR, ch, 0.55))
    for w, files in zip(forms[1:], out[1:]):
        for i, (f, r) in enumerate(zip(files, out[0])):
            if f != r:
                pf, pr = flofile.parse(f), flofile.parse(r)
                msg = describe_data_difference(f"{tag} form {w} against form {forms[0]}, clip {i}", pf.data, pr.data, ch)
                raise AssertionError(msg or f"{tag} form {w} clip {i}: header or TOC differs at byte {first_difference(f, r)}")
    return out[0]


@pytest.mark.parametrize("name", [g[0] for g in M.geometry_batches()])
def test_frame_parallel_geometry_equals_the_chain(ctx, name):
    _, ch, lens = next(g for g in M.geometry_batches() if g[0] == name)
    clips = [M.geometry_clip(n, ch, i) for i, n in enumerate(lens)]
    files = forms_agree(ctx, name, clips, ch)
    for f, n in zip(files, lens):
        p = flofile.parse(f)
        assert p.crc_valid and len(p.frames) == M.hops_of(n)


@pytest.mark.parametrize("frames", M.HANDOVER_FRAMES)
def test_coefficient_hand_over_last_and_first_without(ctx, frames):
    n = (frames - 1) * 1024 - 7
    assert M.hops_of(n) == frames
    want = "Pair2FromCoef" if frames == M.HANDOVER_FRAMES[0] else "Pair2"
    assert ("plan:frames:Pair1," + want) in M.batch_paths(2, [n], 2)
    forms_agree(ctx, f"handover_{frames}", [M.geometry_clip(n, 2, 1)], 2)


# ------------------------------------------------------------------------------------------------ levels that do not decay
_level, _pattern = {}, {}
CLEAN = "clean"


def level_reference(ctx, name):
    """-> (pcm, the form-1 file, channels); name: a case of lossy_model.level_cases, or clean_ch1 / clean_ch2 (nothing replaced)"""
    if name not in _level:
        if name.startswith(CLEAN):
            ch, v, f = int(name[-1]), None, 2
        else:
            _, ch, v, f = next(c for c in M.level_cases() if c[0] == name)
        pcm = M.level_clip(ch, v, f)
        with forced(ctx, 1):
            ref = ctx.encode_lossy(pcm, SR, ch, 0.55)
        _level[name] = (pcm, ref, ch)
    return _level[name]


def level_refs_at(ctx, name, qs):
    """the form-1 files of the clip at the qualities qs"""
    pcm, ref, ch = level_reference(ctx, name)
    out = []
    for q in qs:
        key = (name, q)
        if key not in _level:
            with forced(ctx, 1):
                _level[key] = ref if q == 0.55 else ctx.encode_lossy(pcm, SR, ch, q)
        out.append(_level[key])
    return out


def mixed_names(ch, n):
    """n clip names of one channel count: clean clips between the cases, so that neighbours in a batch differ"""
    cases = [c[0] for c in M.level_cases() if c[1] == ch]
    cycle = [f"{CLEAN}_ch{ch}"]
    for i, c in enumerate(cases):
        cycle.append(c)
        if i % 2:
            cycle.append(f"{CLEAN}_ch{ch}")
    return [cycle[i % len(cycle)] for i in range(n)]


def empty_pattern(file, ch):
    p = flofile.parse(file)
    return np.array([[b == M.EMPTY_BLOB for b in blobs] for _, blobs in M.split_frames(p.data, ch)], bool)


def assert_same_file(tag, got, ref, ch):
    if got != ref:
        pg, pr = flofile.parse(got), flofile.parse(ref)
        msg = describe_data_difference(tag, pg.data, pr.data, ch)
        raise AssertionError(msg or f"{tag}: header or TOC differs at byte {first_difference(got, ref)}")


LEVELS = [c[0] for c in M.level_cases()]


@pytest.mark.parametrize("name", LEVELS)
def test_level_that_does_not_decay_every_form(ctx, name):
    pcm, ref, ch = level_reference(ctx, name)
    want = M.oracle_empty_pattern(pcm, ch)       # (the oracle walks 221 frames: a second or two per case, once)
    got = empty_pattern(ref, ch)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, "form 1: blob empty / oracle all zero differ at (frame, channel)", bad[:8].tolist(),
                           "frames with an empty channel 0:", int(got[:, 0].sum()), "oracle:", int(want[:, 0].sum()))
    for which in (2, 5, 0):
        with forced(ctx, which):
            f = ctx.encode_lossy(pcm, SR, ch, 0.55)
        assert_same_file(f"{name} form {which} against form 1", f, ref, ch)


@pytest.mark.parametrize("which", [0, 2, 5], ids=["auto", "form2", "form5"])
@pytest.mark.parametrize("ch", [1, 2])
def test_level_that_does_not_decay_batch_of_64(ctx, ch, which):
    """every case of this channel count and clean clips between them in one batch: each file is its own clip's form-1
    file, so a mark must belong to its clip, channel and band and to nothing else"""
    names = mixed_names(ch, 64)
    assert set(names) == {c[0] for c in M.level_cases() if c[1] == ch} | {f"{CLEAN}_ch{ch}"}
    clips = [level_reference(ctx, n)[0] for n in names]
    with forced(ctx, which):
        files = ctx.encode_batch(1, clips, SR, ch, 0.55)
    for i, n in enumerate(names):
        assert_same_file(f"batch of 64, {ch} ch, form {which}, clip {i} ({n})", files[i], level_reference(ctx, n)[1], ch)


@pytest.mark.parametrize("ch", [1, 2])
def test_level_marks_of_an_earlier_encode_of_the_batch_are_ignored(ctx, ch):
    """one Batch encoded three times under form 2: a 3e38 clip, a clean clip, the 3e38 clip again. The marks are never
    cleared; an encode reads only those of its own tag."""
    bad, clean = f"3e38_ch{ch}", f"{CLEAN}_ch{ch}"
    pcm = level_reference(ctx, bad)[0]
    b = flo_amd.Batch(ctx, 1, [pcm.size], SR, ch, 0.55)
    try:
        for step, n in enumerate((bad, clean, bad, clean)):
            b.upload(0, level_reference(ctx, n)[0])
            b.encode(2)
            b.sync()
            assert_same_file(f"encode {step} of one batch ({n})", b.fetch(0), level_reference(ctx, n)[1], ch)
    finally:
        b.close()


@pytest.mark.parametrize("groups", ["one_group", "a_group_per_clip"])
@pytest.mark.parametrize("ch", [1, 2])
def test_level_that_does_not_decay_curve_and_ladder(ctx, ch, groups):
    """all cases and clean clips in one batch; with a group limit of 1 MiB every clip is a group of its own (a clip larger
    than the limit), so the marks of a later group are indexed from that group's first clip"""
    names = mixed_names(ch, 11)
    qs = [0.35, 0.55, 0.75]
    refs = [level_refs_at(ctx, n, qs) for n in names]
    clips = [level_reference(ctx, n)[0] for n in names]
    limit = None if groups == "one_group" else 1 << 20
    b = flo_amd.Batch(ctx, 1, [c.size for c in clips], SR, ch, 0.55)
    try:
        for i, c in enumerate(clips):
            b.upload(i, c)
        with forced(ctx, 0, FLO_SIZE_CURVE_GROUP_BYTES=limit, FLO_LADDER_GROUP_BYTES=limit):
            curve = b.size_curve(qs)
            lad = b.encode_ladder(qs)
        try:
            for i, n in enumerate(names):
                assert [int(x) for x in curve[i]] == [len(r) for r in refs[i]], (n, i, "size curve against the form-1 files")
                for j, q in enumerate(qs):
                    assert_same_file(f"clip {i} ({n}) ladder rung {j} (q {q})", lad.fetch(i, j), refs[i][j], ch)
        finally:
            lad.close()
    finally:
        b.close()


@pytest.mark.parametrize("push", [1, 130, 0], ids=["1_frame", "130_frames", "all_at_once"])
@pytest.mark.parametrize("name", LEVELS)
def test_level_that_does_not_decay_streaming(ctx, name, push):
    pcm, ref, ch = level_reference(ctx, name)
    e = flo_amd.LossyStreamingEncoder(SR, ch, 0.55, ctx)
    try:
        step = (push * 1024 * ch) or pcm.size
        for a in range(0, pcm.size, step):
            e.push_samples(pcm[a:a + step])
        assert_same_file(f"{name} streamed in pushes of {push or 'all'} frames", e.finalize(), ref, ch)
    finally:
        e.close()


@pytest.mark.parametrize("ch", [1, 2])
def test_level_that_does_not_decay_encode_streams(ctx, ch):
    """every case and clean streams between them in the same encode_streams calls, cut at frame 100: for the cases of frames
    2 and 70 the carried level is all that remembers the frame when frame 130 is encoded; each stream keeps its own"""
    names = mixed_names(ch, 11)
    cut = 100 * 1024 * ch
    es = [flo_amd.LossyStreamingEncoder(SR, ch, 0.55, ctx) for _ in names]
    try:
        for part in (slice(0, cut), slice(cut, None)):
            for e, n in zip(es, names):
                e.append_samples(level_reference(ctx, n)[0][part])
            r = flo_amd.encode_streams(es, ctx)
            assert not r.status.any(), r.errors
        for i, (e, n) in enumerate(zip(es, names)):
            assert_same_file(f"encode_streams stream {i} ({n})", e.finalize(), level_reference(ctx, n)[1], ch)
    finally:
        for e in es:
            e.close()


def test_transform_encoder_keeps_a_level_that_does_not_decay(ctx):
    """TransformEncoder.encode_frame keeps 65 spectra of history; frame 140 of a clip with 2e19 in frame 2 must still be what
    the sequential chain over all 141 spectra gives (channel 0 empty), and the clean channel what it is without the sample"""
    pcm = level_reference(ctx, "2e19_ch2")[0].reshape(-1, 2)
    n = 141
    enc = flo_amd.TransformEncoder(SR, 2, 0.55, ctx)
    blocks = [np.ascontiguousarray(pcm[1024 * h:1024 * h + 2048]).reshape(-1) for h in range(n)]
    for b in blocks:
        last = enc.encode_frame(b)
    spectra = np.stack([ctx.mdct_forward(np.ascontiguousarray(b.reshape(2048, 2).T).reshape(-1)) for b in blocks])
    with forced(ctx, 1):
        want = ctx.lossy_quantize(spectra, SR, 0.55)
    assert not want["q"][-1, 0].any() and want["q"][-1, 1].any()
    for c in range(2):
        assert np.array_equal(np.asarray(last.coefficients[c]), want["q"][-1, c]), ("channel", c)
