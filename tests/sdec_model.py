"""A restatement of libflo's StreamingDecoder (libflo/src/streaming/decoder.rs) in Python: the state machine, the counters
and the frame parser statement by statement, and the decode of each frame. Test infrastructure: the expected model for
flo_amd.StreamingDecoder. Frame decode comes from the oracle: a lossless frame through oracle.decode_lossless_i32 of a
one-frame file, a transform frame through deserialize_sparse + mdct_inverse with the overlap kept here.

Frames the device decoder declines (see include/flo_hip.h) are reported as Unsupported errors, as the product does."""
import struct

import numpy as np

from fixtures_util import dequantise
from oracle import oracle as O

WAITING_HEADER, WAITING_TOC, READY, FINISHED, ERROR = range(5)


class ModelError(Exception):
    pass


def parse_alpc_channel(d):
    """parse_alpc_channel (:427-473) -> dict or raises ModelError"""
    if not d:
        return {"coeffs": [], "shift": 0, "enc": 2, "k": 0, "res": b""}
    order = d[0]
    if order > 12:
        raise ModelError("Invalid LPC order")
    if len(d) < 1 + order * 4 + 2:
        raise ModelError("ALPC channel too small")
    coeffs = list(struct.unpack_from("<%di" % order, d, 1))
    pos = 1 + order * 4
    shift, enc = d[pos], d[pos + 1]
    pos += 2
    k = 0
    if enc == 0:
        if pos >= len(d):
            raise ModelError("Missing rice parameter")
        k = d[pos]
        pos += 1
    return {"coeffs": coeffs, "shift": shift, "enc": enc, "k": k, "res": d[pos:]}


def parse_frame(data, channels):
    """parse_frame (:356-425) -> (type, samples, flags, [channel])"""
    if len(data) < 6:
        raise ModelError("Frame too small")
    ft, ns, fl = struct.unpack_from("<BIB", data, 0)
    n = 1 if ft == 253 else channels
    pos = 6
    chans = []
    for _ in range(n):
        if pos + 4 > len(data):
            raise ModelError("Frame truncated")
        cs = struct.unpack_from("<I", data, pos)[0]
        pos += 4
        if pos + cs > len(data):
            raise ModelError("Channel data truncated")
        cd = data[pos:pos + cs]
        pos += cs
        if ft == 0:
            chans.append(None)
        elif ft in (253, 254):
            chans.append(cd)
        else:
            chans.append(parse_alpc_channel(cd))
    return ft, ns, fl, chans


def classify_blob(b, channels):
    """deserialize_frame (lossy/decoder.rs:61-131): 'none', 'unsupported' (device: non-Long or too many channels) or 'ok'"""
    if len(b) < 2 or b[0] > 3:
        return "none"
    nch = b[1]
    pos = 2 + 50 * nch
    if pos > len(b):
        return "none"
    for _ in range(nch):
        if pos + 4 > len(b):
            return "none"
        ln = struct.unpack_from("<I", b, pos)[0]
        pos += 4
        if pos + ln > len(b):
            return "none"
        pos += ln
    return "unsupported" if (b[0] != 0 or nch > channels) else "ok"


class StreamingDecoderModel:
    def __init__(self):
        self.reset()

    def reset(self):
        self.buffer = bytearray()
        self.state = WAITING_HEADER
        self.header = None
        self.toc = []
        self.current = 0
        self.data_offset = 0
        self.is_lossy = False
        self.skipped_preroll = False
        self.overlap = None

    # -- public surface
    def feed(self, data):
        """True / False, or raises ModelError on bad magic"""
        if self.state in (ERROR, FINISHED):
            return False
        self.buffer += bytes(data)
        return self._advance()

    def info(self):
        if self.header is None:
            return None
        h = self.header
        return (h["sample_rate"], h["channels"], h["bit_depth"], h["total_samples"], self.is_lossy)

    def frames_available(self):
        return self._count_complete() if self.state == READY else 0

    def available_frames(self):
        return max(self._count_complete() - self.current, 0) if self.state == READY else 0

    def snapshot(self):
        return (self.state, self.frames_available(), self.available_frames(), len(self.buffer), self.info())

    def next_frame(self):
        """np.float32 array, None, or raises ModelError (without advancing)"""
        if self.state != READY:
            return None
        if self.current >= len(self.toc):
            self.state = FINISHED
            return None
        s, e = self._span(self.current)
        if e > len(self.buffer):
            return None
        ch = self.header["channels"]
        ft, ns, fl, chans = parse_frame(bytes(self.buffer[s:e]), ch)
        out = self._decode(ft, ns, fl, chans, bytes(self.buffer[s:e]))
        self.current += 1
        return out

    # -- internals
    def _advance(self):
        while True:
            if self.state == WAITING_HEADER:
                if not self._parse_header():
                    return False
                self.state = WAITING_TOC
                continue
            if self.state == WAITING_TOC:
                if not self._parse_toc():
                    return False
                self.state = READY
                return True
            if self.state == READY:
                return self._count_complete() > self.current
            return False

    def _parse_header(self):
        if len(self.buffer) < 70:
            return False
        b = bytes(self.buffer[:70])
        if b[:4] != b"FLO!":
            self.state = ERROR
            raise ModelError("Invalid flo file: bad magic")
        flags, sr, ch, bd, total = struct.unpack_from("<HIBBQ", b, 6)
        self.header = {"flags": flags, "sample_rate": sr, "channels": ch, "bit_depth": bd, "total_samples": total,
                       "toc_size": struct.unpack_from("<Q", b, 38)[0]}
        self.is_lossy = bool(flags & 1)
        self.overlap = np.zeros((ch, 1024), np.float32)
        return True

    def _parse_toc(self):
        ts = self.header["toc_size"]
        end = 70 + ts
        if len(self.buffer) < end:
            return False
        if ts >= 4:
            n = struct.unpack_from("<I", self.buffer, 70)[0]
            for i in range(n):
                o = 74 + 20 * i
                if o + 20 > len(self.buffer):
                    return False
                self.toc.append(struct.unpack_from("<IQII", self.buffer, o))   # frame_index, byte_offset, frame_size, ts
        self.data_offset = end
        return True

    def _span(self, i):
        e = self.toc[i]
        s = self.data_offset + e[1]
        return s, s + e[2]

    def _count_complete(self):
        n = 0
        for i in range(len(self.toc)):
            if self._span(i)[1] <= len(self.buffer):
                n += 1
            else:
                break
        return n

    def _decode(self, ft, ns, fl, chans, raw):
        h = self.header
        ch = h["channels"]
        if ft == 253:
            if not self.is_lossy:
                raise ModelError("Unsupported: transform frame in a lossless stream")
            blob = chans[0]
            cls = classify_blob(blob, ch)
            if cls == "unsupported":
                raise ModelError("Unsupported: transform block")
            if cls == "none":
                return np.zeros(0, np.float32)
            pcm = self._transform(blob)
            if not self.skipped_preroll:
                self.skipped_preroll = True
                return np.zeros(0, np.float32)
            return pcm
        if self.is_lossy:
            raise ModelError("Unsupported: non-transform frame in a lossy stream")
        if ns > 2000000:
            raise ModelError("Unsupported: frame samples")
        for c in chans:
            if isinstance(c, dict) and c["coeffs"] and c["enc"] != 0:
                raise ModelError("Unsupported: raw ALPC residuals")
        if ch == 0:
            return np.zeros(0, np.float32)
        return self._lossless(ft, ns, fl, chans, raw)

    def _transform(self, blob):
        """TransformDecoder::decode_frame (lossy/decoder.rs:29-52) + overlap-add (mdct.rs:449-456), one Long block"""
        h = self.header
        ch = h["channels"]
        band = O.psy_tables(h["sample_rate"])[1]
        nb = blob[1]
        words = np.frombuffer(blob, "<u2", count=25 * nb, offset=2).reshape(nb, 25)
        pos = 2 + 50 * nb
        out = np.zeros((1024, ch), np.float32)
        for c in range(nb):
            ln = struct.unpack_from("<I", blob, pos)[0]
            q = np.asarray(O.deserialize_sparse(blob[pos + 4:pos + 4 + ln]), np.float32)
            pos += 4 + ln
            spec = dequantise(q, words[c], band).astype(np.float32)
            rec = np.asarray(O.mdct_inverse(spec), np.float32)
            out[:, c] = rec[:1024] + self.overlap[c]
            self.overlap[c] = rec[1024:]
        return out.reshape(-1)

    def _lossless(self, ft, ns, fl, chans, raw):
        """decode_frame's lossless half (:502-538) through the oracle's decoder on a one-frame file (the channel wrappers
        re-serialised as ALPC / silence so that the file reader sees what parse_frame saw)"""
        h = self.header
        ch = h["channels"]
        body = bytearray(struct.pack("<BIB", 1, ns, fl))
        for c in chans:
            if c is None:   # silence: order 0, raw encoding, no residuals
                w = bytes([0, 0, 2])
            elif isinstance(c, (bytes, bytearray)):   # raw: order 0, raw encoding, the i16 pairs
                w = bytes([0, 0, 2]) + bytes(c)
            else:
                w = bytes([len(c["coeffs"])]) + struct.pack("<%di" % len(c["coeffs"]), *c["coeffs"])
                w += bytes([c["shift"], 0, c["k"]]) if c["enc"] == 0 else bytes([c["shift"], c["enc"]])
                w += bytes(c["res"])
            body += struct.pack("<I", len(w)) + w
        toc = struct.pack("<I", 1) + struct.pack("<IQII", 0, 0, len(body), 0)
        head = b"FLO!" + struct.pack("<BBHIBBQB", 1, 2, 0, h["sample_rate"], ch, 16, ns, 5) + b"\0\0\0"
        head += struct.pack("<IQQQQQ", 0, 66, len(toc), len(body), 0, 0)
        ints = O.decode_lossless_i32(head + toc + bytes(body))[0].reshape(-1)
        return ints.astype(np.float32) * np.float32(1.0 / 32767.0)
