"""Header, TOC and CRC32 of every finished file (launch_finish_files and its kernels in container_kernels.hip,
crc_slice_reg in crc_device.hpp, tail_crc in lossy_kernels.hip) against tests/container_model.py, on the cases whose
paths tests/test_container_model_cpu.py accounts for. For every file of every case:

  1. bytes 0 .. 74 + 20 nf equal the model's header and TOC written from the frames and the DATA bytes the device
     returned, field by field; a failure names the field or TOC entry, the clip and the clip's path names;
  2. the CRC field equals zlib.crc32 of the DATA bytes the device returned (so a CRC failure is neither masked by nor
     blamed on an encoder difference);
  3. the whole file equals the oracle's.

The many-clips stereo case runs as tests/test_gpu_tail_crc.py does: the tail on, a second epoch, the tail off (every CRC
from crc_fallback_256) and form 1 (crc_slices_kernel); all four must give the same files.

Its clips are silent: a lossy file with non-zero coefficients equals the oracle's only within the transform's tolerance,
not byte for byte. container_model.tone_case, 34 tone clips among 256, has a test of its own with checks 1 and 2 and the
four makers' agreement, with the path names taken from the DATA lengths the device returned, and asserts that those
lengths still take the two NT = 64 paths that only an odd length reaches.

What the host does to a finished file on the way out (META appended, meta_size and a lossless file's bit depth patched)
is checked for the three fetchers at the end.
"""
import zlib

import pytest

import container_model as M
import flofile
from gpu_util import ctx  # noqa: F401
from test_gpu_tail_crc import _encode, _files

pytestmark = pytest.mark.gpu

CASES = [c["name"] for c in M.cases()]


def check_files(name, what, got, want, paths):
    """want: the oracle's files, or None per file where only the model and zlib are asked. The model's header comes from the
    case's parameters and its TOC from walking the returned DATA frame by frame, not from the device's header or TOC."""
    assert len(got) == len(want), (name, what)
    c = M.case(name)
    for i, (g, w) in enumerate(zip(got, want)):
        tag = f"{name} ({what}) clip {i}, paths {sorted(paths[i])}"
        try:
            head = M.model_head(g, M.case_header(c, i))
        except Exception as e:      # the device's own header or TOC does not even split the file: show it against the oracle's
            diff = repr(e)
            if w is not None:
                head = w[:74 + 20 * len(flofile.parse(w).frames)]
                diff = M.head_difference(g[:len(head)], head) or diff
            raise AssertionError(f"{tag}: the file does not parse: {diff}")
        diff = M.head_difference(g[:len(head)], head)
        assert diff is None, f"{tag}: {diff}"
        p = flofile.parse(g)
        crc = zlib.crc32(p.data) & 0xFFFFFFFF
        assert p.data_crc32 == crc, f"{tag}: CRC field {p.data_crc32:#010x}, zlib over the returned DATA {crc:#010x} ({p.data_size} bytes)"
        if w is not None and g != w:
            at = next((k for k in range(min(len(g), len(w))) if g[k] != w[k]), min(len(g), len(w)))
            raise AssertionError(f"{tag}: differs from the oracle's file at byte {at} of {len(g)} / {len(w)} (DATA starts at {len(head)})")


def make_batch(ctx, c, pcm):
    import flo_amd
    mode = flo_amd.MODE_LOSSLESS if c["kind"] == "lossless" else flo_amd.MODE_LOSSY
    qol = c["qol"] if c["kind"] != "ladder" else c["qualities"][0]
    b = flo_amd.Batch(ctx, mode, [p.size for p in pcm], c["sr"], c["ch"], qol)
    for i, p in enumerate(pcm):
        b.upload(i, p)
    return b


def packed_files(b, sizes):
    """every finished file through flo_batch_pack_files -> [bytes]"""
    import torch
    buf = torch.zeros(sum(sizes) + 16 * len(sizes) + 1024, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    offs = b.pack_files(buf.data_ptr(), buf.numel())
    b.sync()
    host = buf.cpu().numpy()
    return [host[offs[i]:offs[i] + sizes[i]].tobytes() for i in range(len(sizes))]


@pytest.mark.parametrize("name", CASES)
def test_finished_files_equal_the_model_and_the_oracle(ctx, name):
    c = M.case(name)
    pcm, want, paths = M.pcm_of(name), M.oracle_files(name), M.case_clip_paths(name)
    b = make_batch(ctx, c, pcm)
    try:
        if c["kind"] == "ladder":
            lad = b.encode_ladder(c["qualities"])
            try:
                got = [lad.fetch(i, j) for j in range(lad.n_rungs) for i in range(lad.n_clips)]
            finally:
                lad.close()
            check_files(name, "ladder, rung-major", got, [f for rung in want for f in rung], paths)
            return
        if len(c["variants"]) > 1:      # many stereo clips: four makers of the same files
            first = _encode(b)
            check_files(name, "tail on", first, want, paths)
            assert _encode(b) == first, f"{name}: the second epoch gives other files"
            fallback = _encode(b, tail=False)
            check_files(name, "tail off: crc_fallback_256", fallback, want, paths)
            b.encode(1)
            b.sync()
            check_files(name, "form 1: crc_slices_kernel", _files(b), want, paths)
            _encode(b)      # (the batch's result for pack_files below is the chain form's again)
        else:
            b.encode(0)
            b.sync()
            check_files(name, "batch", _files(b), want, paths)
        if c["pack"]:
            check_files(name, "pack_files", packed_files(b, [len(w) for w in want]), want, paths)
    finally:
        b.close()


def test_tone_clips_in_the_chain_form_equal_the_model_under_every_maker(ctx):
    c = M.tone_case()
    name, n = c["name"], len(c["clips"])
    b = make_batch(ctx, c, M.pcm_of(name))

    def paths_of(files, which, tail):       # from the device's own lengths and frames
        return M.batch_paths(M.batch_of("lossy", c["ch"], files, which=which, tail=tail))
    try:
        first = _encode(b)
        tail_paths = paths_of(first, 5, True)
        check_files(name, "tail on", first, [None] * n, tail_paths)
        assert _encode(b) == first, f"{name}: the second epoch gives other files"
        assert _encode(b, tail=False) == first, f"{name}: crc_fallback_256 gives other files"
        b.encode(1)
        b.sync()
        assert _files(b) == first, f"{name}: form 1 (crc_slices_kernel) gives other files"
    finally:
        b.close()
    # what the clips are here for. The lengths equal the oracle's (container_model.FOUND_DATA); should a change of the
    # encoder's rounding move them, search FOUND again: nothing else runs tail_crc's last-63 and one-byte branches
    sizes = [flofile.parse(f).data_size for f in first[:2]]
    assert sizes == [M.FOUND_DATA["lossy_stereo_16385"], M.FOUND_DATA["lossy_stereo_last63"]], sizes
    assert {"nt64:one_byte", "nt256:one_byte", "layout:one_byte_over_a_boundary"} <= tail_paths[0] | paths_of(first, 5, False)[0]
    assert "nt64:last63" in tail_paths[1]
    assert {"nt64:last63", "nt64:one_byte"} <= set().union(*tail_paths)


@pytest.mark.parametrize("kind", ["lossless", "lossy", "ladder"])
def test_fetch_appends_meta_and_patches_the_header(ctx, kind):
    """Every fetcher (flo_batch_fetch of a lossless and of a lossy batch, flo_ladder_fetch): the file fetched with META is
    the file fetched without, with META behind it and its length at bytes 62 .. 69; a lossless file's byte 13 is the
    batch's bit depth."""
    import struct

    import numpy as np

    import flo_amd
    rng = np.random.default_rng(7)
    pcm = [(0.25 * rng.standard_normal(2 * n)).astype(np.float32) for n in (1, 1025, 3000)]
    metas = [b"", b"\x80", bytes(range(256)) + bytes(44)]
    mode = flo_amd.MODE_LOSSLESS if kind == "lossless" else flo_amd.MODE_LOSSY
    b = flo_amd.Batch(ctx, mode, [p.size for p in pcm], 44100, 2, {"lossless": 5, "lossy": 0.55, "ladder": 0.35}[kind])
    lad = None
    try:
        for i, p in enumerate(pcm):
            b.upload(i, p)
        if kind == "ladder":
            lad = b.encode_ladder([0.35, 1.0])
            fetchers = [lambda m, i=i, j=j: lad.fetch(i, j, m) for i in range(3) for j in range(2)]
        else:
            if kind == "lossless":
                b.set_bit_depth(24)
            b.encode(0)
            b.sync()
            fetchers = [lambda m, i=i: b.fetch(i, m) for i in range(3)]
        for k, fetch in enumerate(fetchers):
            plain = fetch(b"")
            assert flofile.parse(plain).crc_valid, (kind, k)
            assert plain[62:70] == bytes(8), (kind, k)
            if kind == "lossless":
                assert plain[13] == 24, (kind, k)
            for m in metas:
                assert fetch(m) == plain[:62] + struct.pack("<Q", len(m)) + plain[70:] + m, (kind, k, len(m))
    finally:
        if lad is not None:
            lad.close()
        b.close()
