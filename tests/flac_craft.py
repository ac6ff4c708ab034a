"""A small deterministic FLAC *writer* -- TEST TOOLING ONLY.

Given samples and a recipe it emits a valid stream with correct CRC-8, CRC-16 and MD5; the recipe sets the block sizes and,
per subframe, the type, order, coefficients, precision, shift, partition order, Rice parameters and escapes, wasted bits, and
the channel assignment.  The samples are known before encoding, so expected values exist by construction; every crafted
stream is first decoded by tests/tools/flac_decode.py (an independent reader) and has to give the samples back
(`crafted_set`).  `malformed_set` derives the broken streams from well-formed ones.

A subframe recipe is a dict:
    type        "constant" | "verbatim" | "fixed" | "lpc" | an int (a raw 6-bit type code: reserved ones for the malformed set)
    order       FIXED 0..4 / LPC 1..32
    coefs, precision, shift   LPC only
    wasted      wasted bits (the samples must have them clear)
    method      0 (4-bit Rice parameters) | 1 (5-bit)
    porder      partition order
    params      one entry per partition: k, or ("esc", raw_bits); a single entry is repeated; None = the smallest k per partition
A frame recipe is a dict: blocksize, assignment (0..7 independent, 8 left/side, 9 side/right, 10 mid/side), subframes (one
recipe per channel, or one for all), bs_code (force block-size code 6 or 7).
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))

FIXED = {0: (), 1: (1,), 2: (2, -1), 3: (3, -3, 1), 4: (4, -6, 4, -1)}


class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, k):
        if k:
            self.acc = (self.acc << k) | (int(v) & ((1 << k) - 1))
            self.n += k

    def unary(self, q):
        self.put(1, q + 1)

    def pad(self):
        self.put(0, -self.n % 8)

    def bytes(self):
        assert self.n % 8 == 0
        return self.acc.to_bytes(self.n // 8, "big")


def crc8(data):
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_CRC16 = []
for _i in range(256):
    _c = _i << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC16.append(_c)


def crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


def utf8_number(v):
    if v < 0x80:
        return bytes([v])
    n = 2
    while v >= 1 << (5 * n + 1) and n < 7:   # n bytes carry 5n + 1 bits
        n += 1
    out = [0x80 | ((v >> (6 * i)) & 0x3F) for i in range(n - 1)][::-1]
    return bytes([((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))] + out)


def _residual(bw, res, blocksize, order, sf):
    method, porder = sf.get("method", 0), sf.get("porder", 0)
    pbits = 5 if method else 4
    bw.put(method, 2)
    bw.put(porder, 4)
    psize = blocksize >> porder
    params = sf.get("params")
    if not isinstance(params, (list, tuple)) or (len(params) == 2 and params[0] == "esc"):
        params = [params] * (1 << porder)
    pos = 0
    for part in range(1 << porder):
        cnt = psize - (order if part == 0 else 0)
        assert cnt >= 0 or sf.get("force"), "the first partition is shorter than the predictor order"
        chunk = res[pos:pos + max(cnt, 0)]
        pos += max(cnt, 0)
        k = params[part]
        if k is None:   # smallest total size
            zz = [(r << 1) ^ (r >> 63) for r in chunk]
            k = min(range(15 if not method else 31), key=lambda kk: sum((z >> kk) + 1 + kk for z in zz)) if zz else 0
        if isinstance(k, tuple):
            nb = k[1]
            bw.put((1 << pbits) - 1, pbits)
            bw.put(nb, 5)
            for r in chunk:
                assert (nb == 0 and r == 0) or (nb and -(1 << (nb - 1)) <= r < (1 << (nb - 1))), (r, nb)
                bw.put(r, nb)
        else:
            bw.put(k, pbits)
            for r in chunk:
                z = (r << 1) if r >= 0 else ((-r) << 1) - 1
                bw.unary(z >> k)
                bw.put(z, k)


def _subframe(bw, s, bps, sf):
    """s: this channel's samples of the block (python ints), bps: the subframe's depth (side channels: + 1)"""
    typ, wasted = sf.get("type", "fixed"), sf.get("wasted", 0)
    order = sf.get("order", 2 if typ == "fixed" else 0)
    if typ in ("fixed", "lpc") and len(s) <= order:   # a short last block
        typ = "verbatim"
    code = {"constant": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 31 + order}.get(typ, typ)
    bw.put(0, 1)
    bw.put(code, 6)
    bw.put(1 if wasted else 0, 1)
    if wasted:
        assert all(x % (1 << wasted) == 0 for x in s)
        bw.unary(wasted - 1)
        s = [x >> wasted for x in s]
        bps -= wasted
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1))
    assert all(lo <= x < hi for x in s), "a sample does not fit the subframe's depth"
    if typ == "constant":
        assert len(set(s)) == 1
        bw.put(s[0], bps)
    elif typ == "verbatim" or not isinstance(typ, str):
        for x in s:
            bw.put(x, bps)
    else:
        for x in s[:order]:
            bw.put(x, bps)
        if typ == "lpc":
            coefs, prec, shift = sf["coefs"], sf["precision"], sf["shift"]
            assert len(coefs) == order and all(-(1 << (prec - 1)) <= c < (1 << (prec - 1)) for c in coefs)
            bw.put(prec - 1, 4)
            bw.put(shift, 5)
            for c in coefs:
                bw.put(c, prec)
        else:
            coefs, shift = FIXED[order], 0
        res = [s[i] - (sum(c * s[i - 1 - j] for j, c in enumerate(coefs)) >> max(shift, 0)) for i in range(order, len(s))]
        assert all(-(1 << 31) < r < (1 << 31) for r in res)
        _residual(bw, res, len(s), order, sf)


_BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
_SS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}


def frame(samples, bps, number, variable, fr, ss_code=None):
    """samples: [blocksize][channels] python ints; returns the frame's bytes"""
    n, ch = len(samples), len(samples[0])
    assign = fr.get("assignment", ch - 1)
    code = fr.get("bs_code") or _BS_CODES.get(n) or (6 if n <= 256 else 7)
    head = Bits()
    head.put(0x3FFE, 14)
    head.put(0, 1)
    head.put(1 if variable else 0, 1)
    head.put(code, 4)
    head.put(0, 4)   # sample rate: see STREAMINFO
    head.put(assign, 4)
    head.put(_SS_CODES.get(bps, 0) if ss_code is None else ss_code, 3)
    head.put(0, 1)
    hb = head.bytes() + utf8_number(number)
    if code == 6:
        hb += bytes([n - 1])
    elif code == 7:
        hb += (n - 1).to_bytes(2, "big")
    hb += bytes([crc8(hb)])
    cols = [[row[c] for row in samples] for c in range(ch)]
    depth = [bps] * ch
    if assign == 8:
        cols, depth = [cols[0], [a - b for a, b in zip(*cols)]], [bps, bps + 1]
    elif assign == 9:
        cols, depth = [[a - b for a, b in zip(*cols)], cols[1]], [bps + 1, bps]
    elif assign == 10:
        cols, depth = [[(a + b) >> 1 for a, b in zip(*cols)], [a - b for a, b in zip(*cols)]], [bps, bps + 1]
    subs = fr.get("subframes", {})
    subs = subs if isinstance(subs, list) else [subs] * len(cols)
    bw = Bits()
    for c, col in enumerate(cols):
        _subframe(bw, col, depth[c], subs[c])
    bw.pad()
    body = hb + bw.bytes()
    return body + crc16(body).to_bytes(2, "big")


def stream(samples, bps, frames, rate=44100, variable=False, first_number=0, id3=False, extra_blocks=(), total_known=True,
           zero_md5=False, min_frame_known=True, ss_code=None, streaminfo_bps=None):
    """samples: int array [n] or [n, channels]; frames: a list of frame recipes, or one recipe (dict with "blocksize") that is
    repeated to the end.  Returns (file bytes, frame table [(offset, nbytes, first_sample, blocksize)])."""
    a = np.asarray(samples, dtype=np.int64)
    a = a.reshape(len(a), -1)
    rows = a.tolist()
    n, ch = a.shape
    if isinstance(frames, dict):
        bs = frames["blocksize"]
        frames = [dict(frames, blocksize=min(bs, n - p)) for p in range(0, n, bs)]
    blobs, table, pos = [], [], 0
    for i, fr in enumerate(frames):
        bs = fr["blocksize"]
        number = first_number + pos if variable else first_number + i
        blobs.append(frame(rows[pos:pos + bs], bps, number, variable, fr, ss_code))
        table.append((0, len(blobs[-1]), pos, bs))
        pos += bs
    assert pos == n, (pos, n)
    width = (bps + 7) // 8
    le = a.astype("<i8").reshape(-1).view(np.uint8).reshape(-1, 8)[:, :width].tobytes()
    md5 = bytes(16) if zero_md5 else hashlib.md5(le).digest()
    sizes = [t[3] for t in table]
    body_sizes = sizes[:-1] or sizes
    si = Bits()
    si.put(min(body_sizes), 16)
    si.put(max(sizes), 16)
    si.put(min(len(b) for b in blobs) if min_frame_known else 0, 24)
    si.put(max(len(b) for b in blobs) if min_frame_known else 0, 24)
    si.put(rate, 20)
    si.put(ch - 1, 3)
    si.put((streaminfo_bps or bps) - 1, 5)
    si.put(n if total_known else 0, 36)
    blocks = [(0, si.bytes() + md5)] + list(extra_blocks)
    out = b""
    if id3:
        tag = b"TIT2" + (6).to_bytes(4, "big") + b"\0\0" + b"\0craft"
        out += b"ID3\x04\x00\x00" + bytes([0, 0, 0, len(tag)]) + tag
    out += b"fLaC"
    for k, (typ, body) in enumerate(blocks):
        out += bytes([typ | (0x80 if k == len(blocks) - 1 else 0)]) + len(body).to_bytes(3, "big") + body
    table2 = []
    for blob, (_, nb, first, bs) in zip(blobs, table):
        table2.append((len(out), nb, first, bs))
        out += blob
    return out, table2


# ---------------------------------------------------------------------------------------------------------------------------------
# the crafted set: the smallest shapes at which the decoder can go wrong

def _rng_samples(seed, n, ch, bps, scale=1.0):
    rng = np.random.default_rng(seed)
    lim = int(((1 << (bps - 1)) - 1) * scale)
    walk = np.cumsum(rng.integers(-max(1, lim // 64), max(1, lim // 64) + 1, size=(n, ch)), axis=0)
    return np.clip(walk, -lim - 1, lim).astype(np.int64)


def _lpc(order, precision, shift, **kw):
    top = (1 << (precision - 1)) - 1
    coefs = [(top if j % 2 == 0 else -top - 1) >> (j // 2 if precision > 4 else 0) for j in range(order)]
    return dict(type="lpc", order=order, coefs=coefs, precision=precision, shift=shift, **kw)


def crafted_set():
    """[(name, file bytes, samples [n, channels], bps, frame table)] -- built once per process."""
    global _CRAFTED
    if _CRAFTED is not None:
        return _CRAFTED
    out = []

    def add(name, samples, bps, frames, **kw):
        a = np.asarray(samples, np.int64)
        a = a.reshape(len(a), -1)
        data, table = stream(a, bps, frames, **kw)
        out.append((name, data, a, bps, table))

    # block sizes and frame counts; frame numbers in 1, 2 and 3 bytes
    for nfr in (1, 63, 64, 65, 129):
        add(f"frames{nfr}", _rng_samples(nfr, 16 * nfr, 1, 16), 16, dict(blocksize=16))
    add("frames2049", _rng_samples(7, 16 * 2049, 1, 8), 8, dict(blocksize=16, subframes=dict(type="fixed", order=1)))
    for k, bs in enumerate((192, 4096, 4608)):
        add(f"bs{bs}", _rng_samples(20 + k, 2 * bs + 1, 2, 16), 16, dict(blocksize=bs))   # ... and a last frame of 1 sample
    add("bs_code6", _rng_samples(30, 200 + 17, 1, 16), 16, dict(blocksize=200))
    add("bs_code7_small", _rng_samples(31, 3 * 16, 1, 16), 16, dict(blocksize=16, bs_code=7))
    add("bs65535", np.full((65535 + 5, 1), -3), 8, dict(blocksize=65535, subframes=dict(type="constant")))
    # three songs of 70 + 1 + 58 frames: a wavefront spans songs
    for k, nfr in enumerate((70, 1, 58)):
        add(f"span{nfr}", _rng_samples(40 + k, 192 * nfr - 5, 2, 16), 16, dict(blocksize=192, assignment=8 + k))
    # variable block size, sample numbers past 2^31 (a file cut out of a longer stream)
    sizes = [16, 4096, 192, 17, 1]
    add("variable_past_2_31", _rng_samples(50, sum(sizes), 1, 16), 16, [dict(blocksize=b) for b in sizes], variable=True,
        first_number=(1 << 31) - 20)
    add("variable_past_2_35", _rng_samples(51, sum(sizes), 2, 16), 16, [dict(blocksize=b) for b in sizes], variable=True,
        first_number=(1 << 35) + 12345)
    # every subframe type, FIXED 0..4, LPC orders / precision / shift
    n = 64
    add("constant_verbatim", np.stack([np.full(n, 1234), _rng_samples(60, n, 1, 16)[:, 0]], 1), 16,
        dict(blocksize=n, assignment=1, subframes=[dict(type="constant"), dict(type="verbatim")]))
    for order in range(5):
        add(f"fixed{order}", _rng_samples(61 + order, 2 * n + 3, 1, 16, 0.02), 16, dict(blocksize=n, subframes=dict(type="fixed", order=order)))
    for order, prec, shift in ((1, 1, 0), (2, 15, 14), (8, 15, 14), (12, 12, 10), (13, 12, 10), (31, 15, 14), (32, 15, 14), (32, 5, 0)):
        add(f"lpc{order}_p{prec}_s{shift}", _rng_samples(70 + order + prec, 3 * n, 1, 16, 0.01), 16,
            dict(blocksize=n, subframes=_lpc(order, prec, shift, method=1)))
    # 24-bit, order 32, precision 15 on full-scale samples: the sum wraps 32 bits
    full = np.where(np.arange(4 * n) % 2 == 0, (1 << 23) - 1, -(1 << 23)).reshape(-1, 1)
    add("lpc32_wrap24", full, 24, dict(blocksize=n, subframes=dict(type="lpc", order=32, precision=15, shift=15, method=1,
                                                                   coefs=[16383 if j % 2 == 0 else -16384 for j in range(32)],
                                                                   params=("esc", 31))), )
    # Rice coding: parameters 0 and 14, 5-bit parameters up to 30, escapes, partition orders, unary runs
    runs = [0, 31, 32, 63, 64, 65, 200]
    unary = np.array([(q >> 1) if q % 2 == 0 else -((q + 1) >> 1) for q in runs] + [0] * 9).reshape(-1, 1)
    add("unary_runs", unary, 16, dict(blocksize=16, subframes=dict(type="fixed", order=0, params=0)))
    add("rice14", _rng_samples(80, 32, 1, 16), 16, dict(blocksize=32, subframes=dict(type="fixed", order=1, params=14)))
    add("rice5bit30", _rng_samples(81, 32, 1, 24), 24, dict(blocksize=32, subframes=dict(type="fixed", order=0, method=1, params=30)))
    add("escapes", np.concatenate([np.zeros(8), [0, 0, -1, -1, 0, -1, 0, 0], _rng_samples(82, 8, 1, 16)[:, 0], _rng_samples(83, 8, 1, 24)[:, 0]]).reshape(-1, 1),
        24, dict(blocksize=32, subframes=dict(type="fixed", order=0, porder=2, params=[("esc", 0), ("esc", 1), ("esc", 16), ("esc", 24)])))
    add("porder_max", _rng_samples(84, 64, 1, 16), 16, dict(blocksize=64, subframes=dict(type="fixed", order=0, porder=6)))
    add("porder15", np.full((32768, 1), 0), 8, dict(blocksize=32768, subframes=dict(type="fixed", order=0, porder=15, params=0)))
    add("first_partition_empty", _rng_samples(85, 64, 1, 16, 0.01), 16, dict(blocksize=64, subframes=dict(type="fixed", order=4, porder=4)))
    # wasted bits, depths, channels
    add("wasted1", _rng_samples(86, 48, 2, 16, 0.4) * 2, 16, dict(blocksize=16, assignment=1, subframes=dict(type="fixed", order=2, wasted=1)))
    add("wasted7", _rng_samples(87, 48, 1, 16, 0.005) * 128, 16, dict(blocksize=16, subframes=dict(type="fixed", order=1, wasted=7)))
    for bps in (8, 12, 16, 20, 24):
        add(f"depth{bps}", _rng_samples(90 + bps, 40, 2, bps), bps, dict(blocksize=16, assignment=10))
    for ch in (1, 2, 3, 8):
        add(f"channels{ch}", _rng_samples(100 + ch, 40, ch, 16), 16, dict(blocksize=16, assignment=ch - 1))
    # all four stereo modes with odd and negative side values and both extreme sample values
    for bps in (16, 24):
        lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
        ext = np.array([[hi, lo], [lo, hi], [hi, hi], [lo, lo], [0, -1], [-1, 0], [1, -2], [-3, 4], [hi, 0], [0, lo], [lo, 1], [hi - 1, lo + 2],
                        [5, 5], [-7, -8], [lo, -1], [hi, 1]])
        for assign in (1, 8, 9, 10):
            add(f"stereo{assign}_{bps}", ext, bps, dict(blocksize=16, assignment=assign, subframes=dict(type="verbatim")))
    # containers and metadata
    base = _rng_samples(110, 3 * 192, 2, 16)
    add("id3", base, 16, dict(blocksize=192), id3=True)
    add("meta_blocks", base, 16, dict(blocksize=192),
        extra_blocks=[(1, bytes(40)), (3, bytes(18 * 2)), (6, (3).to_bytes(4, "big") + bytes(28) + b"\xff\xf8\xc9\x18\x00" * 3), (4, bytes(8))])
    add("total_unknown", base, 16, dict(blocksize=192), total_known=False)
    add("md5_zero", base, 16, dict(blocksize=192), zero_md5=True)
    # bytes behind the audio (an ID3v1 tag): the last frame of the table runs to the end of the data, the decoder stops before
    data, table = stream(base, 16, dict(blocksize=192))
    tag = b"TAG" + b"\xff\xf8craft".ljust(125, b"\0")
    out.append(("trailing_id3v1", data + tag, base, 16, table[:-1] + [(table[-1][0], table[-1][1] + len(tag), table[-1][2], table[-1][3])]))
    # the fooling stream: a VERBATIM subframe carries a byte-perfect frame header with a valid CRC-8 and the expected next number
    fake = b"\xff\xf8" + bytes([(6 << 4) | 0, (0 << 4) | (4 << 1)]) + utf8_number(1) + bytes([15])
    fake += bytes([crc8(fake)])
    fake += b"\x00" * (len(fake) % 2)
    words = np.frombuffer(fake, ">i2").astype(np.int64)
    fool = _rng_samples(120, 3 * 16, 1, 16)
    fool[4:4 + len(words), 0] = words
    add("fooling", fool, 16, dict(blocksize=16, subframes=dict(type="verbatim")), min_frame_known=False)
    _CRAFTED = out
    return out


_CRAFTED = None
FOOLING = "fooling"


def malformed_set():
    """[(name, file bytes)]: every one of them has to end in a decode error, none in a fault."""
    good = {name: (data, table) for name, data, _, _, table in crafted_set()}
    data, table = good["bs192"]
    out = [("not_flac", b"RIFF" + data[4:]), ("garbage", bytes(range(256)) * 8), ("empty", b"")]
    out.append(("cut_in_metadata", data[:20]))
    out.append(("cut_in_header", data[:table[1][0] + 3]))
    out.append(("cut_in_residual", data[:table[1][0] + table[1][1] // 2]))
    out.append(("cut_before_footer", data[:-2]))
    out.append(("cut_at_frame_boundary", data[:table[2][0]]))
    s = _rng_samples(130, 32, 1, 16, 0.01)
    out.append(("reserved_subframe_type", stream(s, 16, dict(blocksize=16, subframes=dict(type=5)))[0]))
    out.append(("reserved_subframe_type_lpc_gap", stream(s, 16, dict(blocksize=16, subframes=dict(type=20)))[0]))
    out.append(("reserved_assignment", stream(np.stack([s[:, 0], s[:, 0]], 1), 16, dict(blocksize=16, assignment=11))[0]))
    out.append(("negative_shift", stream(s, 16, dict(blocksize=16, subframes=dict(type="lpc", order=1, coefs=[1], precision=4, shift=-1)))[0]))
    out.append(("depth32", stream(s, 32, dict(blocksize=16, subframes=dict(type="verbatim")))[0]))
    out.append(("depth32_frame_only", stream(s, 16, dict(blocksize=16, subframes=dict(type="verbatim")), ss_code=7)[0]))
    out.append(("partition_shorter_than_order", stream(s, 16, dict(blocksize=16, subframes=dict(type="fixed", order=4, porder=3, force=True)))[0]))
    return out
