"""A model of the decisions the parallel lossless decoder takes (flo_amd/csrc/lldec_kernels.hip, ll_route / LlWrapperList
in ll_route.cpp, ll_finish_kernel in decode_kernels.hip), in plain integers. It restates what the kernels do, not what
the format says: the oracle stays the checker of values (tests/test_lldec_model_cpu.py holds the model to it).

* route() / WrapperList: ll_route and LlWrapperList::push, expression for expression (pinned to the native dump).
* scan(): ll_rice_scan_kernel - per tile and entry state where the parse stands at the frontier, the leaders, the exit
  state and the codes started (the `tabs` word); scan_geometry() its wavefronts and workgroups.
* chain(): ll_rice_chain_kernel - tile_entry per tile and the total of codes (the tail behind it is cleared).
* residual_tile(): one lane of ll_rice_decode_kernel - the values, the iterations, skip / esc / lost.
* predict(): ll_predict_kernel - which form takes each wrapper; for the row form the group, MAXO, the super-blocks on
  the unpredicated path and the largest magnitude the wavefront sees (run-on over zero residuals included), hence the
  device's serial flag. Exact integers: the f64 form is exact until the flag is already due.
* finish(): ll_finish_kernel - vector or scalar, quads and tail, mid/side, the floats.
* decode(): all of it for a file: integers, floats, the paths reached (names of PATHS) and the wrappers handed to the
  serial kernel by the host and by the device.
* PATHS / NOT_REACHED / cases() / case(name): the table of paths and the files that reach them.

What the model shows about the handover by magnitude: `worst` holds |sample|, so a sample equal to INT_MIN (|s| = 2^31) is
handed over although it is representable - a needless serial decode, not a wrong value; INT_MAX and -INT_MAX are not."""
import struct

import numpy as np

import flofile

TILE_BITS = 1024          # kRiceTileBits
STATES = 16               # kRiceStates
MAX_K = STATES - 2        # kRiceMaxK
SCAN_WAVES = 8            # kScanWaves
FRONTIER = 192            # FLO_SCAN_FRONTIER
SCAN_GRID_TILES = SCAN_WAVES * 4   # the scan's grid is sized for kScanTiles = 4 tiles per wavefront (k = 14)
CHAIN_CHUNK = 256         # kChainChunk
DEC_OVER = 16             # kDecOver
DEC_WAVE_TILES = 64       # tiles per workgroup of ll_rice_decode_kernel
SB = 16                   # kSb
ESCAPE = 256              # ones that end a unary run without a terminator
CSUM_LIMIT = 1 << 21      # sum |coef| the f64 recurrence takes
SHIFT_LIMIT = 20
LEN_CAP = 16 * 1024 * TILE_BITS   # payload bytes above which ll_route sends a Rice wrapper to the serial kernel
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
T = TILE_BITS


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


# ---- route -----------------------------------------------------------------------------------------------------------
def wrapper(k=0, coeffs=(), shift=0, payload=b"", samples=0):
    return dict(k=int(k), coeffs=[int(c) for c in coeffs], shift=int(shift) & 0xFF, payload=bytes(payload), samples=int(samples))


def route(w, force_serial=False, length=None):
    """ll_route: (serial, other, tiles). `length` stands in for len(payload) (the cap needs no 16 MiB of bytes)."""
    ln = len(w["payload"]) if length is None else length
    nco, sh, k = len(w["coeffs"]), w["shift"], w["k"]
    rice = ln > 0 and (nco > 0 or sh >= 128)
    csum = sum(abs(c) for c in w["coeffs"])
    ser = force_serial or (rice and k > MAX_K) or csum >= CSUM_LIMIT or (nco > 0 and (sh & 63) > SHIFT_LIMIT)
    if rice and ln > LEN_CAP:
        ser = True
    other = not (0 < nco <= 12 and ln > 0 and w["samples"] > nco)
    tiles = (ln + T // 8 - 1) // (T // 8) if rice and not ser else 0
    return int(bool(ser)), int(other), tiles


class WrapperList:
    """LlWrapperList: tile0, serial, others, out_off per wrapper, scratch, max_tiles"""

    def __init__(self):
        self.ws, self.tile0, self.serial, self.others, self.out_off, self.frames = [], [0], [], [], [], []
        self.scratch = self.max_tiles = self.max_samples = 0

    def push(self, w, r):
        i = len(self.ws)
        self.ws.append(w)
        self.out_off.append(self.scratch)
        self.scratch += w["samples"]
        self.serial.append(r[0])
        if r[1]:
            self.others.append(i)
        self.tile0.append(self.tile0[-1] + r[2])
        self.max_tiles = max(self.max_tiles, r[2])
        return i

    def add_frame(self, out_off, samples, mid_side, ws, force_serial=False):
        fr = dict(out_off=out_off, first=len(self.ws), n_channels=len(ws), samples=samples, mid_side=int(bool(mid_side)), scratch_off=[0, 0])
        for k, w in enumerate(ws):
            w = dict(w, samples=samples)
            if k < 2:
                fr["scratch_off"][k] = self.scratch
            self.push(w, route(w, force_serial))
        self.max_samples = max(self.max_samples, samples)
        self.frames.append(fr)


def wrappers_of(flo, force_serial=False):
    """file_ll_wrappers: the wrapper list flo_decode builds for a lossless file -> (WrapperList, channels, sample-frames)"""
    f = flofile.parse(flo)
    L = WrapperList()
    at = 0
    for fr in f.frames:
        ws = []
        for c in fr.channels:
            if 1 <= fr.frame_type <= 12:
                ws.append(wrapper(c.rice_k if c.encoding == 0 else 0, c.coeffs, c.shift_bits, c.residuals))
            elif fr.frame_type == 254:
                ws.append(wrapper(payload=c.raw[:2 * fr.frame_samples]))
            else:
                ws.append(wrapper())
        L.add_frame(at, fr.frame_samples, f.channels == 2 and (fr.flags & 1), ws, force_serial)
        at += fr.frame_samples
    return L, f.channels, at


# ---- the stream: bits behind `len` are zeros (be_word) -------------------------------------------------------------------
def bit_string(payload, tiles):
    n = 8 * len(payload)
    s = bin(int.from_bytes(payload, "big"))[2:].zfill(n) if n else ""
    return s + "0" * ((tiles + DEC_WAVE_TILES + 1) * T + 32 * DEC_OVER + 64 - n)


def _look(s, at):
    """the window of 32 bits at `at`: leading ones (32 for a window of ones)"""
    z = s.find("0", at, at + 32)
    return 32 if z < 0 else z - at


# ---- 1. tile tables --------------------------------------------------------------------------------------------------------
def _scan_step(s, base, pos, k):
    ones = _look(s, base + pos)
    z = pos + ones
    in_tile = z < T
    term = in_tile and ones < 32
    npos = (z if in_tile else T + k + 1) + (k + 1 if term else 0)
    return npos, int(term and npos < T)


def scan_tile(s, t, k):
    """One tile of ll_rice_scan_kernel -> dict(front = [(pos, n)] per entry state after phase 1, leader = [state] per entry
    state (None: no candidate), leaders = the leading states, tabs = [(exit state, codes started)] per entry state)"""
    base = t * T
    front = []
    for st in range(k + 2):
        pos, n = (st, 1) if st <= k else (0, 0)
        while pos < FRONTIER:
            pos, d = _scan_step(s, base, pos, k)
            n += d
        front.append((pos, n))
    leader, walked = [], {}
    for st, (pos, n) in enumerate(front):
        if pos >= T:
            leader.append(None)
            continue
        lead = next(j for j in range(st + 1) if front[j][0] == pos)
        leader.append(lead)
        if lead == st:
            p2, n2 = pos, 0
            while p2 < T:
                p2, d = _scan_step(s, base, p2, k)
                n2 += d
            walked[st] = (p2 - T, n2)
    tabs = []
    for st, (pos, n) in enumerate(front):
        if leader[st] is None:
            tabs.append((pos - T, n))
        else:
            ex, n2 = walked[leader[st]]
            tabs.append((ex, n + n2))
    return dict(front=front, leader=leader, leaders=sorted(walked), tabs=tabs)


def scan_geometry(k, nt, max_tiles):
    """the scan's grid for one wrapper: tiles per wavefront, active and surplus workgroups, and per active workgroup the
    tiles of each of its eight wavefronts"""
    tpw = 64 // (k + 2)
    grid = (max_tiles + SCAN_GRID_TILES - 1) // SCAN_GRID_TILES
    wgs = []
    for y in range(grid):
        t0g = y * SCAN_WAVES * tpw
        if t0g >= nt:
            continue
        wgs.append([max(0, min(tpw, nt - (t0g + wv * tpw))) for wv in range(SCAN_WAVES)])
    return dict(tpw=tpw, grid=grid, active=len(wgs), surplus=grid - len(wgs), waves=wgs)


def scan(w, tiles, max_tiles):
    s = bit_string(w["payload"], tiles)
    k = w["k"]
    tl = [scan_tile(s, t, k) for t in range(tiles)]
    g = scan_geometry(k, tiles, max_tiles)
    per = SCAN_WAVES * g["tpw"]
    g["wg_leaders"] = [sum(len(x["leaders"]) for x in tl[y * per:(y + 1) * per]) for y in range(g["active"])]
    return dict(bits=s, tiles=tl, geometry=g)


# ---- 2. the chain ------------------------------------------------------------------------------------------------------------
def chain(tabs, samples):
    """-> dict(entry = [(index of the first code, entry state)] per tile, chunk per tile, total, cleared = samples the
    kernel zeroes behind the last code)"""
    st = idx = 0
    entry = []
    for tb in tabs:
        entry.append((idx, st))
        st, d = tb[st]
        idx += d
    return dict(entry=entry, chunk=[t // CHAIN_CHUNK for t in range(len(tabs))], total=idx, cleared=(min(idx, samples), samples))


# ---- 3. residuals ----------------------------------------------------------------------------------------------------------
def residual_tile(s, t, k, entry, n):
    """One lane of ll_rice_decode_kernel -> dict(first, values, iters, skip, esc ('q' / 'limit' / None), lost,
    over = a code of this tile reads its bits behind the 64 staged tiles)"""
    idx, st = entry
    wave0 = (t // DEC_WAVE_TILES) * DEC_WAVE_TILES * T
    tile_lo, tile_hi = t * T, (t + 1) * T
    limit = wave0 + DEC_WAVE_TILES * T + 32 * (DEC_OVER - 2)
    skip = st == k + 1
    was_skip = skip
    pos = tile_lo + (0 if skip else st)
    active = skip or (pos < tile_hi and idx < n)
    first, q, values, iters, esc, lost, over = idx, 0, [], 0, None, False, False
    while active:
        iters += 1
        ones = _look(s, pos)
        z, q2 = pos + ones, q + ones
        term = ones < 32
        e = (not skip) and (q2 >= ESCAPE or z >= limit)
        if e:
            esc = "q" if q2 >= ESCAPE else "limit"
        if skip and z >= tile_hi:
            lost = True
        emit = term and not skip and not e
        if emit:
            rem = int(s[z + 1:z + 1 + k], 2) if k else 0
            u = (q2 << k) | rem
            values.append((u >> 1) ^ -(u & 1))
            idx += 1
            if z + 1 + k > wave0 + DEC_WAVE_TILES * T:
                over = True
        npos = z + 1 + k if term else z
        go_on = (not e) and (not lost) and ((npos < tile_hi and idx < n) if term else True)
        pos, q, skip = npos, (0 if term else q2), (skip and not term)
        active = go_on
    return dict(first=first, values=values, iters=iters, skip=was_skip, esc=esc, lost=lost, over=over)


def rice_stage(w, tiles, max_tiles):
    """scan, chain and the residual stage of one wrapper -> dict(residuals (what the scratch holds behind the stage: None
    where nothing was written), escaped, scan, chain, lanes)"""
    sc = scan(w, tiles, max_tiles)
    ch = chain([x["tabs"] for x in sc["tiles"]], w["samples"])
    n = w["samples"]
    out = [None] * n
    for i in range(*ch["cleared"]):
        out[i] = 0
    lanes = []
    for t in range(tiles):
        r = residual_tile(sc["bits"], t, w["k"], ch["entry"][t], n)
        r["no_code_start"] = sc["tiles"][t]["tabs"][ch["entry"][t][1]][1] == 0
        for j, v in enumerate(r["values"]):
            out[r["first"] + j] = v
        lanes.append(r)
    waves = [lanes[i:i + DEC_WAVE_TILES] for i in range(0, tiles, DEC_WAVE_TILES)]
    iters = [max(x["iters"] for x in wv) for wv in waves]
    return dict(residuals=out, escaped=any(x["esc"] for x in lanes), scan=sc, chain=ch, lanes=lanes, wave_iters=iters,
                flushes=[i // 16 + 1 for i in iters])


# ---- the reader, as the serial kernel and the format have it (rice_next / reconstruct_*) ----------------------------------------
def rice_read(payload, k, n):
    s = bin(int.from_bytes(payload, "big"))[2:].zfill(8 * len(payload)) if payload else ""
    L, pos, out = len(s), 0, []
    for _ in range(n):
        if pos >= L:
            out.append(0)
            continue
        z = s.find("0", pos, pos + ESCAPE)
        if z < 0:
            q = min(ESCAPE, L - pos)
            pos += q
        else:
            q = z - pos
            pos = z + 1
        rem = 0
        if k <= 32:
            bits = s[pos:pos + k]
            rem = int(bits.ljust(k, "0"), 2) if k else 0
            pos = min(L, pos + k)
        else:
            for _ in range(k):
                bit = 0
                if pos < L:
                    bit = int(s[pos])
                    pos += 1
                rem = ((rem << 1) | bit) & 0xFFFFFFFF
        u = ((q << (k & 31)) | rem) & 0xFFFFFFFF
        out.append(_i32((u >> 1) ^ -(u & 1)))
    return out


def serial_decode(w):
    """ll_decode_kernel for one wrapper: i32 arithmetic with wrap-around"""
    n, nco, sh = w["samples"], len(w["coeffs"]), w["shift"]
    p = w["payload"]
    if not nco and p and sh >= 128:
        r = rice_read(p, w["k"], n)
        order = sh - 128
        out = []
        for i, rv in enumerate(r):
            eff = min(0 if order > 4 else order, i)
            h = [out[i - j] if i - j >= 0 else 0 for j in range(1, 5)]
            pred = (0, h[0], 2 * h[0] - h[1], 3 * h[0] - 3 * h[1] + h[2], 4 * h[0] - 6 * h[1] + 4 * h[2] - h[3])[eff]
            out.append(_i32(rv + pred))
        return out
    if nco:
        r = rice_read(p, w["k"], n)
        out = []
        for i, rv in enumerate(r):
            v = rv
            if i >= nco:
                pred = sum(w["coeffs"][j] * out[i - 1 - j] for j in range(nco))
                v = _i32(_i32(pred >> (sh & 63)) + rv)
            out.append(v)
        return out
    if p:
        pairs = len(p) // 2
        return [struct.unpack_from("<h", p, 2 * i)[0] if i < pairs else 0 for i in range(n)]
    return [0] * n


# ---- 4. predictors -----------------------------------------------------------------------------------------------------------
def takes_rows(w, serial):
    nco = len(w["coeffs"])
    return (not serial) and 0 < nco <= 12 and len(w["payload"]) > 0 and w["samples"] > nco


def rows_blocks(nmax):
    """blocks predict_rows steps (whole super-blocks, the dummy block nb included) for the longest wrapper of a group"""
    nb = (nmax + 15) >> 4
    return nb, SB * ((nb + 1 + SB - 1) // SB)


def rows_unpredicated(nmin, nmax):
    """the super-blocks whose loads and stores take the unpredicated path"""
    nb, blocks = rows_blocks(nmax)
    out = []
    sb = 0
    while SB * sb < nb + 1 + SB:
        if sb >= 2 and 16 * (SB * (sb + 1) + SB + 1) <= nmin:
            out.append(sb)
        sb += 1
    return out


def lpc_row(res, coeffs, sh, n, count):
    """the recurrence in exact integers over `count` samples (zero residuals behind n) -> (samples [n], index of the first
    sample of magnitude >= 2^31 or None). Nothing behind that index is looked at: the flag is due."""
    order = len(coeffs)
    s, bad = [], None
    for i in range(count):
        v = res[i] if i < n else 0
        if i >= order:
            v += sum(coeffs[j] * s[i - 1 - j] for j in range(order)) >> sh
        if abs(v) >= 2 ** 31:
            bad = i
            break
        s.append(v)
    return s[:n], bad


def predict(L, residuals, flags):
    """ll_predict_kernel over a list. residuals[i]: the scratch of wrapper i behind the Rice stage; flags: the serial flags
    at that point (host and escapes). -> (samples per wrapper (None: left to the serial kernel), forms per wrapper,
    groups, flags behind the kernel)"""
    n_ch = len(L.ws)
    flags = list(flags)
    forms = [None] * n_ch
    out = [None] * n_ch
    groups = []
    before = list(flags)
    for g in range((n_ch + 3) // 4):
        rows = [(4 * g + r < n_ch) and takes_rows(L.ws[4 * g + r], before[4 * g + r]) for r in range(4)]
        if not any(rows):
            groups.append(dict(group=g, rows=rows, maxo=None))
            continue
        ws = [L.ws[4 * g + r] if rows[r] else None for r in range(4)]
        maxo = 12 if any(w and len(w["coeffs"]) > 8 for w in ws) else 8
        ns = [w["samples"] if w else 0 for w in ws]
        nmax, nmin = max(ns), min(x for x, w in zip(ns, ws) if w)
        nb, blocks = rows_blocks(nmax)
        seen = 16 * (blocks - 1)   # block b's first steps read block b - 1 out: blocks 0 .. blocks - 2 reach `worst`
        info = dict(group=g, rows=rows, maxo=maxo, nmin=nmin, nmax=nmax, nb=nb, blocks=blocks, unpredicated=rows_unpredicated(nmin, nmax),
                    in_chain=[4 * g + r < n_ch for r in range(4)], flagged=[None] * 4)
        for r, w in enumerate(ws):
            if not w:
                continue
            i = 4 * g + r
            s, bad = lpc_row(residuals[i], w["coeffs"], w["shift"] & 63, w["samples"], seen)
            forms[i] = "rows%d" % maxo
            if bad is None:
                out[i] = s
            else:
                flags[i] = 1
                info["flagged"][r] = "sample" if bad < w["samples"] else "run-on"
        groups.append(info)
    for i in L.others:
        w = L.ws[i]
        if takes_rows(w, flags[i]):   # (never: `others` are exactly the wrappers the row form does not take)
            continue
        if flags[i]:
            forms[i] = "one:serial"
            continue
        nco, sh, n = len(w["coeffs"]), w["shift"], w["samples"]
        if not nco and w["payload"] and sh >= 128:
            order = sh - 128
            r = list(residuals[i])
            if 1 <= order <= 4:
                forms[i] = "one:fixed%d" % order
                for m in range(order - 1, -1, -1):   # sum m starts at sample m
                    acc = 0
                    for j in range(m, n):
                        acc = _i32(acc + r[j])
                        r[j] = acc
            else:
                forms[i] = "one:copy_order0" if order == 0 else "one:copy_order_over_4"
            out[i] = r
        elif not nco:
            p = w["payload"]
            forms[i] = "one:raw" if p else "one:silent"
            out[i] = [struct.unpack_from("<h", p, 2 * j)[0] if j < len(p) // 2 else 0 for j in range(n)]
        elif not w["payload"]:
            forms[i] = "one:lpc_no_bytes"
            out[i] = [0] * n
        else:
            forms[i] = "one:n<=order"
            out[i] = list(residuals[i])
    for i in range(n_ch):
        if forms[i] is None:
            forms[i] = "serial"   # an LPC wrapper the rows leave alone: flagged before ll_predict
    return out, forms, groups, flags


# ---- 5. finish -----------------------------------------------------------------------------------------------------------------
def finish_form(fr, out_offs, channels):
    """which loop of ll_finish_kernel takes the frame (the float output; decode_lossless_i32 always takes the scalar one)"""
    if channels == 2 and fr["n_channels"] == 2:
        oa, o1 = out_offs[fr["first"]], out_offs[fr["first"] + 1]
        if fr["mid_side"]:
            oa, o1 = fr["scratch_off"]
        if ((oa | o1) & 3) == 0 and (fr["out_off"] & 1) == 0:
            return dict(vector=True, quads=fr["samples"] >> 2, tail=fr["samples"] & 3, mid_side=bool(fr["mid_side"]))
    return dict(vector=False, quads=0, tail=0, mid_side=bool(fr["mid_side"] and fr["n_channels"] == 2))


def _half(v):
    v = _i32(v)
    return -((-v) // 2) if v < 0 else v // 2


def finish(L, planes, channels, frames_total):
    """-> (interleaved i32, interleaved f32, forms per frame, pre-cleared?)"""
    oi = np.zeros(frames_total * channels, np.int64)
    forms = []
    for fr in L.frames:
        f = finish_form(fr, L.out_off, channels)
        forms.append(f)
        n, o = fr["samples"], fr["out_off"]
        if f["mid_side"]:
            m, s = planes[fr["first"]], planes[fr["first"] + 1]
            oi[2 * o:2 * (o + n):2] = [_half(a + b) for a, b in zip(m, s)]
            oi[2 * o + 1:2 * (o + n):2] = [_half(a - b) for a, b in zip(m, s)]
        else:
            for c in range(min(fr["n_channels"], channels)):
                oi[o * channels + c:(o + n) * channels:channels] = planes[fr["first"] + c]
    oi = oi.astype(np.int32)
    of = oi.astype(np.float32) * (np.float32(1.0) / np.float32(32767.0))
    return oi, of, forms, any(fr["n_channels"] < channels for fr in L.frames)


# ---- the whole decode ------------------------------------------------------------------------------------------------------------
def decode(flo):
    """-> dict(i32, f32, host, device, paths, wrappers = per wrapper dict(route, rice, form, flag), groups, frames, list)"""
    L, channels, total = wrappers_of(flo)
    n_ch = len(L.ws)
    flags = list(L.serial)
    res, rice = [None] * n_ch, [None] * n_ch
    for i, w in enumerate(L.ws):
        tiles = L.tile0[i + 1] - L.tile0[i]
        if tiles:
            rice[i] = rice_stage(w, tiles, L.max_tiles)
            res[i] = rice[i]["residuals"]
            if rice[i]["escaped"]:
                flags[i] = 1
    after_rice = list(flags)
    planes, forms, groups, flags = predict(L, res, flags)
    for i, w in enumerate(L.ws):
        if flags[i]:
            planes[i] = serial_decode(w)
        assert planes[i] is not None and None not in planes[i], ("wrapper %d: samples no kernel writes" % i, forms[i])
    oi, of, fforms, cleared = finish(L, planes, channels, total)
    out = dict(i32=oi, f32=of, host=sum(L.serial), device=sum(flags) - sum(L.serial), list=L, channels=channels, groups=groups, frames=fforms,
               wrappers=[dict(route=(L.serial[i], int(i in L.others), L.tile0[i + 1] - L.tile0[i]), rice=rice[i], form=forms[i], flag=flags[i],
                              escaped=bool(after_rice[i] and not L.serial[i]), planes=planes[i]) for i in range(n_ch)], precleared=cleared)
    out["paths"] = paths(out)
    return out


def paths(d):
    """the names of PATHS a decode reaches"""
    p = set()
    L = d["list"]
    for i, w in enumerate(L.ws):
        ser, other, tiles = d["wrappers"][i]["route"]
        nco, sh, k, ln, n = len(w["coeffs"]), w["shift"], w["k"], len(w["payload"]), w["samples"]
        rice_w = ln > 0 and (nco > 0 or sh >= 128)
        csum = sum(abs(c) for c in w["coeffs"])
        if tiles:
            p.add("route:parallel")
        if ser:
            p.add("route:serial_by_host")
        if d["wrappers"][i]["flag"]:
            p.add("route:ll_decode_kernel<1>")
        if rice_w and k == MAX_K:
            p.add("route:k=14")
        if rice_w and k == MAX_K + 1:
            p.add("route:k=15")
        if csum == CSUM_LIMIT - 1:
            p.add("route:csum=2^21-1")
        if csum == CSUM_LIMIT:
            p.add("route:csum=2^21")
        if nco and sh == SHIFT_LIMIT:
            p.add("route:shift=20")
        if nco and sh == SHIFT_LIMIT + 1:
            p.add("route:shift=21")
        if nco and sh == 64 + SHIFT_LIMIT:
            p.add("route:shift=84")
        if not other:
            p.add("route:rows")
        elif nco and n <= nco:
            p.add("route:other_short")
        elif nco and not ln:
            p.add("route:other_no_bytes")
        elif not nco:
            p.add("route:other_fixed" if (ln and sh >= 128) else "route:other_raw" if ln else "route:other_silent")
        r = d["wrappers"][i]["rice"]
        if r:
            g = r["scan"]["geometry"]
            for x in r["scan"]["tiles"]:
                nl = len(x["leaders"])
                p.add("scan:leaders=1" if nl == 1 else "scan:leaders=2+" if nl > 1 else "scan:no_candidate")
            for c in g["wg_leaders"]:
                p.add("scan:wg_leaders=0" if c == 0 else "scan:wg_leaders<=64" if c <= 64 else "scan:wg_leaders>64")
            for wv in g["waves"]:
                for c in wv:
                    p.add("scan:wave_full" if c == g["tpw"] else "scan:wave_idle_in_active_wg" if c == 0 else "scan:last_wave_partial")
            if g["surplus"]:
                p.add("scan:surplus_workgroups")
            per = SCAN_WAVES * g["tpw"]
            for dlt, nm in ((-1, "8tpw-1"), (0, "8tpw"), (1, "8tpw+1")):
                if tiles == per + dlt:
                    p.add("scan:k=%d:tiles=%s" % (k, nm))
            if tiles in (255, 256, 257, 512, 513):
                p.add("chain:tiles=%d" % tiles)
            p.add("chain:one_chunk" if tiles <= CHAIN_CHUNK else "chain:several_chunks")
            ch = r["chain"]
            for t in range(CHAIN_CHUNK, tiles, CHAIN_CHUNK):
                st = ch["entry"][t][1]
                p.add("chain:chunk_starts_on_a_code" if st == 0 else "chain:run_straddles_chunk" if st == k + 1 else "chain:code_straddles_chunk")
            p.add("chain:cleared_tail" if ch["total"] < n else "chain:no_tail")
            if tiles in (63, 64, 65):
                p.add("residual:tiles=%d" % tiles)
            for t, x in enumerate(r["lanes"]):
                if x["over"]:
                    p.add("residual:code_in_the_over_words")
                if x["skip"]:
                    p.add("residual:skip_tile")
                if x["no_code_start"]:
                    p.add("residual:no_code_start")
                if x["lost"]:
                    p.add("residual:lost")
                if x["esc"]:
                    p.add("residual:esc_by_" + ("256_ones" if x["esc"] == "q" else "limit"))
                if not x["iters"]:
                    p.add("residual:tile_behind_the_last_sample")
            for it in r["wave_iters"]:
                p.add("residual:wave_iterations" + ("<16" if it < 16 else "=16" if it == 16 else ">16"))
            if ln % (T // 8) == 0 and w["payload"][-1] & 1:
                last = r["lanes"][-1]
                if last["values"] and not last["esc"]:
                    p.add("residual:stream_ends_in_a_run_at_a_tile_end")
        f = d["wrappers"][i]["form"]
        if f.startswith("one:"):
            p.add("predict:" + f)
    n_ch = len(L.ws)
    for g in d["groups"]:
        if g["maxo"] is None:
            p.add("predict:group_without_rows")
            continue
        p.add("predict:rows_maxo=%d" % g["maxo"])
        orders = [len(L.ws[4 * g["group"] + r]["coeffs"]) for r in range(4) if g["rows"][r]]
        if g["maxo"] == 12 and sum(o > 8 for o in orders) == 1 and len(orders) > 1:
            p.add("predict:rows_maxo=12_by_one_row")
        u = len(g["unpredicated"])
        p.add("predict:rows_unpredicated=" + ("0" if u == 0 else "1" if u == 1 else "2+"))
        if u == 0 and rows_unpredicated(g["nmax"], g["nmax"]):
            p.add("predict:rows_nmin_bars_unpredicated")
        for v in (1039, 1040, 1041, 1295, 1296, 1297):
            if g["nmin"] == v:
                p.add("predict:rows_nmin=%d" % v)
        if not g["rows"][0]:
            p.add("predict:rows_inactive_row_0")
        if not g["rows"][3] and 4 * g["group"] + 3 < n_ch:
            p.add("predict:rows_inactive_row_3")
        if 4 * g["group"] + 3 >= n_ch:
            p.add("predict:rows_last_group_partial")
        for r in range(4):
            if not g["rows"][r]:
                continue
            w = L.ws[4 * g["group"] + r]
            n, o = w["samples"], len(w["coeffs"])
            if n == o + 1:
                p.add("predict:rows_n=order+1")
            if n in (15, 16, 17, 255, 256, 257):
                p.add("predict:rows_n=%d" % n)
            if n < g["nmax"]:
                p.add("predict:rows_shorter_row_runs_on")
            if g["flagged"][r]:
                p.add("predict:rows_flag_by_" + ("sample" if g["flagged"][r] == "sample" else "run-on_only"))
    for f in d["frames"]:
        if f["vector"]:
            p.add("finish:vector_mid_side" if f["mid_side"] else "finish:vector")
            p.add("finish:vector_quads=0" if f["quads"] == 0 else "finish:vector_quads")
            if f["tail"]:
                p.add("finish:vector_tail")
    for fr, f in zip(L.frames, d["frames"]):
        if f["vector"]:
            continue
        if d["channels"] == 2 and fr["n_channels"] == 2:
            p.add("finish:scalar_odd_out_off" if fr["out_off"] & 1 else "finish:scalar_misaligned_scratch")
            p.add("finish:scalar_mid_side" if f["mid_side"] else "finish:scalar_stereo")
        elif fr["n_channels"] < d["channels"]:
            p.add("finish:precleared")
        else:
            p.add("finish:scalar_mono" if d["channels"] == 1 else "finish:scalar_3+_channels")
    return p


PATHS = {
    "route": ["route:parallel", "route:serial_by_host", "route:k=14", "route:k=15", "route:csum=2^21-1", "route:csum=2^21", "route:shift=20",
              "route:shift=21", "route:shift=84", "route:len=cap", "route:len=cap+1", "route:rows", "route:other_short", "route:other_no_bytes",
              "route:other_fixed", "route:other_raw", "route:other_silent", "route:ll_decode_kernel<1>", "route:ll_decode_kernel<0>"],
    "scan": ["scan:leaders=1", "scan:leaders=2+", "scan:no_candidate", "scan:wg_leaders=0", "scan:wg_leaders<=64", "scan:wg_leaders>64",
             "scan:wave_full", "scan:last_wave_partial", "scan:wave_idle_in_active_wg", "scan:surplus_workgroups"] +
            ["scan:k=%d:tiles=%s" % (k, nm) for k in range(MAX_K + 1) for nm in ("8tpw-1", "8tpw", "8tpw+1")],
    "chain": ["chain:tiles=%d" % t for t in (255, 256, 257, 512, 513)] +
             ["chain:one_chunk", "chain:several_chunks", "chain:chunk_starts_on_a_code", "chain:code_straddles_chunk", "chain:run_straddles_chunk",
              "chain:cleared_tail", "chain:no_tail"],
    "residual": ["residual:tiles=63", "residual:tiles=64", "residual:tiles=65", "residual:code_in_the_over_words", "residual:skip_tile",
                 "residual:no_code_start", "residual:lost", "residual:esc_by_256_ones", "residual:esc_by_limit", "residual:tile_behind_the_last_sample",
                 "residual:wave_iterations<16", "residual:wave_iterations=16", "residual:wave_iterations>16",
                 "residual:stream_ends_in_a_run_at_a_tile_end"],
    "predict": ["predict:rows_maxo=8", "predict:rows_maxo=12", "predict:rows_maxo=12_by_one_row", "predict:rows_unpredicated=0",
                "predict:rows_unpredicated=1", "predict:rows_unpredicated=2+", "predict:rows_nmin_bars_unpredicated"] +
               ["predict:rows_nmin=%d" % v for v in (1039, 1040, 1041, 1295, 1296, 1297)] +
               ["predict:rows_inactive_row_0", "predict:rows_inactive_row_3", "predict:rows_last_group_partial", "predict:group_without_rows",
                "predict:rows_n=order+1"] + ["predict:rows_n=%d" % v for v in (15, 16, 17, 255, 256, 257)] +
               ["predict:rows_shorter_row_runs_on", "predict:rows_flag_by_sample", "predict:rows_flag_by_run-on_only"] +
               ["predict:one:fixed%d" % o for o in (1, 2, 3, 4)] +
               ["predict:one:copy_order0", "predict:one:copy_order_over_4", "predict:one:raw", "predict:one:silent", "predict:one:lpc_no_bytes",
                "predict:one:n<=order", "predict:one:serial"],
    "finish": ["finish:vector", "finish:vector_mid_side", "finish:vector_quads", "finish:vector_quads=0", "finish:vector_tail",
               "finish:scalar_misaligned_scratch", "finish:scalar_odd_out_off", "finish:scalar_mid_side", "finish:scalar_stereo", "finish:scalar_mono",
               "finish:scalar_3+_channels", "finish:precleared"],
}
# paths the case table does not reach, each with the reason
NOT_REACHED = {
    "route:len=cap": "a payload of 16 MiB is no small file: the native sweep of tests/native/decode_plan_test.cpp takes ll_route to both sides of the cap",
    "route:len=cap+1": "as route:len=cap: 16 MiB and a byte, taken to ll_route by the native sweep only",
    "route:ll_decode_kernel<0>": "never launched: launch_ll_wrappers always passes `only`, and launch_ll_decode takes the one-wrapper-per-wavefront "
                                 "form whenever `only` is set",
    "scan:no_candidate": "a step of phase 1 starts below the frontier (192) and moves 32 + k + 1 <= 47 bits at most: no parse of a tile the wavefront "
                         "has can stand behind bit 239 at the frontier, let alone behind the tile (1024)",
    "scan:wg_leaders=0": "a workgroup that passes `t0g >= nt` has a tile, and every tile has a candidate (scan:no_candidate)",
    "residual:esc_by_limit": "a code starts below tile_hi <= 65536 and q2 >= 256 fires at the latest with z <= start + 287 < limit = 65984; z >= limit "
                             "needs q2 >= 449, and the lane stopped when q2 reached 256",
    "finish:vector_tail": "LlWrapperList::push gives a frame's two wrappers consecutive runs of the scratch, so o1 = oa + samples: both are multiples "
                          "of four only if samples is, and then no tail is left",
    "finish:vector_quads=0": "as finish:vector_tail: samples is a positive multiple of four on the vector path",
    "finish:precleared": "the container parser gives every frame of a lossless file the header's channel count (a frame of type 253 carries one "
                         "wrapper, but makes the file a transform file), so no hand-made file has a frame with fewer wrappers",
}


# ---- building cases ------------------------------------------------------------------------------------------------------------
class Stream:
    """A Rice stream written code by code, with the bit position known: a value v >= 0 zigzags to 2 v and costs
    (2 v >> k) + 1 + k bits."""

    def __init__(self, k, seed=1, qmax=40):
        self.k, self.bits, self.values, self.pos, self.qmax = k, [], [], 0, qmax
        self.rng = np.random.default_rng(seed)

    def code(self, q, rem=0):
        k = self.k
        self.bits.append("1" * q + "0" + (format(rem, "0%db" % k) if k else ""))
        u = (q << k) | rem
        self.values.append((u >> 1) ^ -(u & 1))
        self.pos += q + 1 + k
        return self

    def fill_to(self, at, qmax=None):
        """random codes while a whole one still ends at or before `at`"""
        k = self.k
        qmax = self.qmax if qmax is None else qmax
        while self.pos + qmax + 1 + k <= at:
            self.code(int(self.rng.integers(0, qmax + 1)), int(self.rng.integers(0, 1 << k)) if k else 0)
        return self

    def land_on(self, at):
        """the next code starts exactly at bit `at`"""
        self.fill_to(at - (self.k + 1) - 1)
        gap = at - self.pos
        if gap:
            assert gap >= self.k + 1, (gap, self.k)
            self.code(gap - 1 - self.k, 0)
        return self

    def run_over(self, at, before=20, after=20):
        """a unary run from `before` bits in front of `at` to `after` bits behind it"""
        self.land_on(at - before)
        return self.code(before + after, (1 << self.k) - 1 if self.k else 0)

    def remainder_over(self, at, back=1):
        """a code whose terminator stands `back` bits in front of `at`: its remainder bits lie on both sides (back <= k)"""
        self.fill_to(at - back - 1)
        return self.code(at - back - self.pos, (1 << self.k) - 1 if self.k else 0)

    def bytes(self, cut=None):
        s = "".join(self.bits)
        s += "0" * (-len(s) % 8)
        b = int(s, 2).to_bytes(len(s) // 8, "big") if s else b""
        return b if cut is None else b[:cut]


def rice_encode(vals, k):
    s = Stream(k)
    for v in vals:
        v = int(v)
        u = (v << 1) ^ (v >> 31) if v >= 0 else ((-v) << 1) - 1
        s.code(u >> k, u & ((1 << k) - 1))
    return s.bytes()


def lpc(coeffs, shift, k, payload):
    return dict(coeffs=[int(c) for c in coeffs], shift=shift, k=k, residuals=bytes(payload))


def fixed(order, k, payload):
    return dict(coeffs=[], shift=128 + order, k=k, residuals=bytes(payload))


def flo_of(frames, channels=1, sr=44100):
    """frames = [(samples, [channel dicts], mid/side flag)]"""
    return flofile.build_lossless(sr, channels, [(8, n, ms, chans) for n, chans, ms in frames])


def _mono(ws):
    return flo_of([(n, [c], 0) for n, c in ws])


def _noise_res(seed, n, k):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.laplace(0, max(0.6, 0.7 * 2.0 ** k), n)), -(100 << k), 100 << k).astype(np.int64)


def _tiles_stream(k, tiles, seed, over=False):
    """a stream of exactly `tiles` tiles (its last byte the last of the tile), one code more than fits whole"""
    s = Stream(k, seed)
    s.fill_to(tiles * T)
    s.code(T if over else 30, 0)   # (cut below: the stream runs out inside it)
    return s, s.bytes(cut=tiles * T // 8)


STABLE = ([1500, -400], 11)
INTEGRATOR = ([1 << 20], 20)


def _cases():
    C = []

    def add(name, group, make):
        C.append(dict(name=name, group=group, make=make))

    # -- route: every limit from both sides, one wrapper each
    def route_limits():
        r = rice_encode(_noise_res(1, 300, 6), 6)
        r14, r15 = rice_encode(_noise_res(2, 300, 14), 14), rice_encode(_noise_res(2, 300, 14), 15)
        return _mono([(300, lpc([900, -100], 10, 14, r14)), (300, lpc([900, -100], 10, 15, r15)), (300, fixed(2, 15, r15)),
                      (300, lpc([CSUM_LIMIT - 5, 4], 20, 6, r)), (300, lpc([CSUM_LIMIT - 4, -4], 20, 6, r)),
                      (300, lpc([900, -100], 20, 6, r)), (300, lpc([900, -100], 21, 6, r)), (300, lpc([900, -100], 84, 6, r)),
                      (300, lpc([900, -100], 85, 6, r)), (300, lpc([CSUM_LIMIT, 0], 10, 6, b""))])
    add("route: k 14 / 15, sum of taps 2^21 - 1 / 2^21, shift 20 / 21 / 84 / 85", "route", route_limits)

    def others():
        r = rice_encode(_noise_res(3, 40, 4), 4)
        ws = [(40, fixed(o, 4, r)) for o in (0, 1, 2, 3, 4, 5, 9)]
        ws += [(40, dict(coeffs=[], shift=0, k=0, residuals=np.arange(-20, 15).astype("<i2").tobytes() + b"\x01")),
               (40, dict(coeffs=[], shift=0, k=0, residuals=b"")), (40, lpc([900, -100], 10, 4, b"")),
               (2, lpc([900, -100], 10, 4, r)), (1, lpc([900, -100], 10, 4, r)), (3, lpc([900, -100], 10, 4, r)),
               (3, fixed(4, 4, r)), (1, fixed(1, 4, r))]
        return _mono(ws)
    add("others: fixed orders 0..5 and 9, raw, silent, taps without bytes, n <= order", "predict", others)

    # -- scan: every k with a tile count at, one below and one above its workgroup's 8 * tpw tiles
    for k in range(MAX_K + 1):
        def geometry(k=k):
            per = SCAN_WAVES * (64 // (k + 2))
            ws = []
            for j, tiles in enumerate((per - 1, per, per + 1)):
                s, b = _tiles_stream(k, tiles, 100 * k + j)
                ws.append((len(s.values) + 3, fixed(0 if k % 2 else 1, k, b)))
            return _mono(ws)
        add("scan k = %d: %d tiles in a workgroup, one fewer, one more" % (k, SCAN_WAVES * (64 // (k + 2))), "scan", geometry)

    # -- chain: tile counts around the chunk, a code and a run over the chunk's boundary
    def chain_case(tiles, how):
        def make():
            s = Stream(14, tiles, qmax=200)
            for b in range(CHAIN_CHUNK, tiles, CHAIN_CHUNK):
                if how == "run":
                    s.run_over(b * T, 100, 100)
                elif how == "code":
                    s.remainder_over(b * T, 5)
                else:
                    s.land_on(b * T)
            s.fill_to(tiles * T)
            s.code(40, 0)
            return _mono([(len(s.values) + 2, lpc(*STABLE, 14, s.bytes(cut=tiles * T // 8)))])
        return make
    for tiles, how in ((255, "none"), (256, "none"), (257, "run"), (257, "code"), (257, "start"), (512, "run"), (513, "run"), (513, "code")):
        add("chain %d tiles, k = 14, %s" % (tiles, dict(none="one chunk", run="a run over the boundary", code="a remainder over the boundary",
                                                         start="a code on the boundary")[how]), "chain", chain_case(tiles, how))

    # -- residual stage
    def staging():
        ws = []
        for tiles in (63, 64, 65):
            s = Stream(14, tiles)
            s.remainder_over(64 * T, 3) if tiles >= 64 else s.fill_to(tiles * T)
            s.fill_to(tiles * T)
            s.code(60, 5)
            ws.append((len(s.values), lpc(*STABLE, 14, s.bytes(cut=tiles * T // 8))))
        return _mono(ws)
    add("residual 63 / 64 / 65 tiles, a remainder in the words behind the 64th", "residual", staging)

    def ones_inside(n_after):
        def make():
            ws = []
            for count in (130, 256, 300):
                for at in (512, 512 + 37):
                    s = Stream(5, count + at)
                    s.fill_to(9 * T)
                    b = bytearray(s.bytes())
                    b[at:at + count] = b"\xff" * count
                    ws.append((len(s.values) if n_after else 40, lpc([900, -100], 10, 5, bytes(b))))
            return _mono(ws)
        return make
    add("ones: 130, 256, 300 bytes of 0xff at tile-aligned and unaligned offsets", "residual", ones_inside(True))
    add("ones behind the last sample: nobody's run, no handover", "residual", ones_inside(False))

    def escape_edge():
        ws = []
        for start in (0, 7, 31, 32, 1000):     # where in the window, and over a tile's end
            for q in (255, 256, 257):
                s = Stream(3, start + q)
                s.land_on(start) if start else None
                s.code(q, 5)
                s.fill_to(s.pos + 600)
                ws.append((len(s.values), fixed(1, 3, s.bytes())))
        return _mono(ws)
    add("escape: runs of 255, 256 and 257 ones", "residual", escape_edge)

    def cut_in_run():
        ws = []
        for tiles, run in ((1, 40), (2, 255), (3, 300), (2, 1)):
            s = Stream(6, tiles * 10 + run)
            s.land_on(tiles * T - run)
            s.code(run + 50, 0)
            ws.append((len(s.values) + 2, lpc(*STABLE, 6, s.bytes(cut=tiles * T // 8))))
        return _mono(ws)
    add("cut: the stream ends inside a run exactly at a tile's end", "residual", cut_in_run)

    def iterations():
        s16 = Stream(14, 5).fill_to(T, 20)   # (runs below 32 ones: one look per code)
        many = bytes(T // 8)   # k = 0: 1024 codes in one tile
        return _mono([(16, lpc(*STABLE, 14, s16.bytes())), (1024, fixed(1, 0, many)), (1030, fixed(0, 0, many + many)), (10, lpc(*STABLE, 14, s16.bytes()))])
    add("flush: 16 iterations, 1024 codes of one bit, fewer than 16", "residual", iterations)

    for k in (0, 1, 7, 14):
        def junk(k=k):
            rng = np.random.default_rng(50 + k)
            b = bytes(rng.integers(0, 256, 700, dtype=np.uint8))
            return _mono([(2500, lpc([1200, -500, 60], 11, k, b)), (2500, fixed(3, k, b))])
        add("random bytes as a stream, k = %d" % k, "residual", junk)

    # -- predictor rows
    def one_row(n, order=4):
        def make():
            taps = np.rint(0.9 * np.array([0.9, -0.5, 0.3, -0.1, 0.05, 0.04, -0.03, 0.02, 0.01, -0.01, 0.005, 0.004][:order]) * 4096).astype(int)
            return _mono([(n, lpc(taps, 12, 6, rice_encode(_noise_res(n, n, 6), 6)))])
        return make
    for n in (1039, 1040, 1041, 1295, 1296, 1297):
        add("rows: one wrapper of %d samples" % n, "predict", one_row(n))
    add("rows: one wrapper of 2100 samples, order 12", "predict", one_row(2100, 12))

    def group_of(ns, orders):
        def make():
            ws = []
            for j, (n, o) in enumerate(zip(ns, orders)):
                r = rice_encode(_noise_res(7 * n + j, n, 5), 5)
                if o:
                    taps = np.rint(0.9 * np.array([0.9, -0.5, 0.3, -0.1, 0.05, 0.04, -0.03, 0.02, 0.01, -0.01, 0.005, 0.004][:o]) * 4096).astype(int)
                    ws.append((n, lpc(taps, 12, 5, r)))
                else:
                    ws.append((n, fixed(2, 5, r)))
            return _mono(ws)
        return make
    add("rows: 500 and 3000 samples share a wavefront", "predict", group_of((500, 3000), (3, 5)))
    add("rows: n = order + 1, 15, 16, 17", "predict", group_of((8, 15, 16, 17), (7, 8, 2, 1)))
    add("rows: n = 255, 256, 257, one row of nine taps", "predict", group_of((255, 256, 257, 100), (8, 1, 9, 4)))
    add("rows: an idle row in front, an idle row behind, a group of none", "predict",
        group_of((60, 70, 80, 90, 90, 80, 70, 60, 30, 30, 30, 30, 50), (0, 3, 12, 4, 5, 6, 7, 0, 0, 0, 0, 0, 10)))

    def edge_of_i32(kind):
        def make():
            big, n = (1 << 21) - 1, 1030
            if kind == "int_max":
                r = [big] * 1024 + [1023] + [0] * 5
            elif kind == "over":
                r = [big] * 1024 + [1024] + [0] * 5
            elif kind == "int_min":
                r = [-(1 << 21)] * 1024 + [0] * 6
            elif kind == "minus_int_max":
                r = [-(1 << 21)] * 1023 + [-(1 << 21) + 1] + [0] * 6
            else:   # under: one below INT_MIN
                r = [-(1 << 21)] * 1024 + [-1] + [0] * 5
            return _mono([(n, lpc(*INTEGRATOR, 14, rice_encode(r, 14)))])
        return make
    add("i32: a sample equal to INT_MAX", "predict", edge_of_i32("int_max"))
    add("i32: a sample equal to -INT_MAX", "predict", edge_of_i32("minus_int_max"))
    add("i32: a sample equal to INT_MIN (handed over by magnitude)", "predict", edge_of_i32("int_min"))
    add("i32: a sample one above INT_MAX", "predict", edge_of_i32("over"))
    add("i32: a sample one below INT_MIN", "predict", edge_of_i32("under"))

    def neighbour():
        # 1039 samples: the row stays off the unpredicated path, whose loads would reach sample 1039 - the next wrapper's first
        # (a copy, no row of the group: nmin stays 1039),
        # 2^21 - 1, enough to take the run-on of a row that rests 3023 below INT_MAX out of the i32 range
        big = (1 << 21) - 1
        a = [big] * 1023 + [big - 2000] + [0] * 15
        return _mono([(1039, lpc(*INTEGRATOR, 14, rice_encode(a, 14))), (20, fixed(0, 14, rice_encode([big] + [0] * 19, 14)))])
    add("run-on: zeros behind the end, not the next wrapper's residuals", "predict", neighbour)

    def run_on(alone):
        def make():
            grow = lpc([2], 0, 4, rice_encode([1] + [0] * 19, 4))     # doubles: 2^19 at its last sample, 2^31 twelve samples on
            if alone:
                return _mono([(20, grow)])
            calm = lpc(*STABLE, 5, rice_encode(_noise_res(9, 900, 5), 5))
            return _mono([(900, calm), (20, grow), (900, calm)])
        return make
    add("run-on: a doubling wrapper of 20 samples alone", "predict", run_on(True))
    add("run-on: a doubling wrapper of 20 samples beside two of 900", "predict", run_on(False))

    # -- finish
    def stereo_lengths():
        frames = []
        for j, n in enumerate((8, 9, 11, 4, 6, 2, 12, 7, 5, 1, 3, 16)):
            chans = [lpc(*STABLE, 12, rice_encode(_noise_res(20 * j + c, n, 4) * 300, 12)) for c in range(2)]
            frames.append((n, chans, j % 3 != 0))
        return flo_of(frames, 2)
    add("finish: stereo frames of 4 m + 0..3 samples in a row", "finish", stereo_lengths)

    def wrapping_pairs():
        # order 1, tap 2^20, shift 0: s1 = s0 * 2^20 + r1 takes any 32-bit value (what follows it wraps on, and is checked too)
        def plane(x):
            return lpc([1 << 20], 0, 14, rice_encode([x[0], x[1], 0, 0], 14))
        top = (2047, (1 << 20) - 1)     # INT_MAX
        low = (-2048, 0)                # INT_MIN
        M = [low, top, (16, 1), top, (0, 1), (33, 3), low, (0, -1), (0, -3)]
        S = [(0, 1), top, (16, 1), low, low, (-33, -3), low, (0, 0), (0, 2)]
        small_m = fixed(0, 3, rice_encode([-1, -3, 1, 0, 7, -8, 5, 5], 3))
        small_s = fixed(0, 3, rice_encode([0, 2, 1, -1, -8, 7, -5, 6], 3))
        frames = [(4, [plane(m), plane(s)], 1) for m, s in zip(M, S)] + [(8, [small_m, small_s], 1)]
        frames += [(4, [plane(m), plane(s)], 0) for m, s in zip(M[:3], S[:3])] + [(3, [small_m, small_s], 1)]
        frames += [(4, [plane(m), plane(s)], 1) for m, s in zip(M, S)]
        return flo_of(frames, 2)
    add("finish: mid/side pairs that wrap, odd and negative; samples above 2^24", "finish", wrapping_pairs)

    def channels_of(ch):
        def make():
            frames = [(n, [lpc(*STABLE, 5, rice_encode(_noise_res(n + c, n, 5), 5)) for c in range(ch)], 1) for n in (9, 4, 30)]
            return flo_of(frames, ch)
        return make
    add("finish: a mono file", "finish", channels_of(1))
    add("finish: a file of three channels", "finish", channels_of(3))
    return C


_CASES = None
_DONE = {}


def cases():
    """[dict(name, group, make)] - make() builds the file (deterministic, not kept); case(name) adds what the model says"""
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


def case(name):
    """-> dict(name, group, flo, paths, host, device, model): the file, the paths the model says it reaches, the wrappers
    the host and the device must hand to the serial kernel, and the whole of decode()"""
    if name not in _DONE:
        c = next(c for c in cases() if c["name"] == name)
        flo = c["make"]()
        d = decode(flo)
        _DONE[name] = dict(name=name, group=c["group"], flo=flo, paths=sorted(d["paths"]), host=d["host"], device=d["device"], model=d)
    return _DONE[name]
