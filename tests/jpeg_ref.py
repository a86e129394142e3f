"""The JPEG side of tests/test_jpeg_transcode.py (TEST INFRASTRUCTURE): a baseline JPEG parser, a float64 decoder written from the
JPEG definition, and the dump of a file's quantised integers that tools/jxlsynth (jpegdata=PATH) turns into a YCbCr VarDCT stream.

This file is the INDEPENDENT side: it imports nothing from ycbcr_ref.py and shares no arithmetic with device/ycbcr_dev.h. Its own
check is a real decoder's output (tests/golden/jpeg/NAME.rgb.npy, written by tools/make_jpeg_fixtures.py with Pillow / libjpeg).

    parse(bytes)                  SOI, APPn, COM, DQT (8-bit), SOF0, DHT, SOS (one interleaved scan of three components), EOI.
                                  Everything else -- progressive, arithmetic, restart intervals, 12 bits, one or four components,
                                  Adobe RGB / CMYK, sampling other than 4:4:4 / 4:2:0 / 4:2:2 / 4:4:0 -- raises ValueError.
    decode_f64(parsed, edge, clamp)  c * Q, the T.81 inverse DCT (A.3.3), + 128, triangle upsampling (3/4, 1/4; horizontal, then vertical;
                                  centred siting), JFIF YCbCr -> RGB. float64 throughout.
    write_dump / transposed / transcoded
"""
import hashlib
import os
import struct
import subprocess

import numpy as np

from streams import SYNTH, CACHE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")

# zigzag position -> natural index 8 v + u (T.81 figure A.6)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

LAYOUTS = {(1, 1): "444", (2, 2): "420", (2, 1): "422", (1, 2): "440"}   # luma's (h, v) with chroma at (1, 1)


class Component:
    def __init__(self, ident, h, v, table, coef):
        self.id, self.h, self.v = ident, h, v
        self.table = table   # uint16 [8, 8], [v, u]: row = vertical frequency
        self.coef = coef     # int16 [blocks_y, blocks_x, 8, 8] over the whole-MCU block grid, [.., v, u], DC differences undone


class Parsed:
    def __init__(self, width, height, components):
        self.width, self.height, self.components = width, height, components
        self.hmax = max(c.h for c in components)
        self.vmax = max(c.v for c in components)
        self.subsampling = LAYOUTS[(components[0].h, components[0].v)]


# ---------------------------------------------------------------- the parser

class _Bits:
    """the entropy-coded segment: 0xFF 0x00 is a data byte 0xFF; any other marker ends the data"""

    def __init__(self, data, at):
        self.d, self.at, self.acc, self.n = data, at, 0, 0

    def bit(self):
        if self.n == 0:
            if self.at >= len(self.d):
                raise ValueError("jpeg: the scan ends before its last MCU")
            b = self.d[self.at]
            if b == 0xFF:
                nxt = self.d[self.at + 1] if self.at + 1 < len(self.d) else 0xD9
                if nxt != 0:
                    if 0xD0 <= nxt <= 0xD7:
                        raise ValueError("jpeg: restart markers are not supported")
                    raise ValueError("jpeg: marker FF%02X inside the scan's data" % nxt)
                self.at += 1
            self.at += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, k):
        v = 0
        for _ in range(k):
            v = v << 1 | self.bit()
        return v


def _huffman(counts, symbols):
    """T.81 annex C: code -> symbol per length, as {(length, code): symbol}"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = symbols[k]
            code += 1; k += 1
        code <<= 1
    return table


def _symbol(br, table):
    code = 0
    for length in range(1, 17):
        code = code << 1 | br.bit()
        s = table.get((length, code))
        if s is not None:
            return s
    raise ValueError("jpeg: a code that is in no Huffman table")


def _extend(v, t):
    return v if t == 0 or v >= 1 << (t - 1) else v - (1 << t) + 1


def parse(data):
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("jpeg: no SOI")
    at, qt, dc_tab, ac_tab, frame = 2, {}, {}, {}, None
    while True:
        if at + 4 > len(data) or data[at] != 0xFF:
            raise ValueError("jpeg: marker expected at byte %d" % at)
        m = data[at + 1]
        if m == 0xFF:
            at += 1
            continue
        if m == 0xD9:
            raise ValueError("jpeg: EOI before a scan")
        size = struct.unpack(">H", data[at + 2:at + 4])[0]
        seg = data[at + 4:at + 2 + size]
        at += 2 + size
        if 0xE0 <= m <= 0xEF or m == 0xFE:
            if m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12 and seg[11] != 1:
                raise ValueError("jpeg: an Adobe file whose components are not YCbCr (RGB or CMYK) is not supported")
        elif m == 0xDB:
            k = 0
            while k < len(seg):
                if seg[k] >> 4:
                    raise ValueError("jpeg: 16-bit quantisation tables (a 12-bit file) are not supported")
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = np.frombuffer(seg[k + 1:k + 65], np.uint8)
                qt[seg[k] & 15] = t.reshape(8, 8)
                k += 65
        elif m == 0xC0:
            if seg[0] != 8:
                raise ValueError("jpeg: %d-bit samples are not supported" % seg[0])
            height, width, nf = struct.unpack(">HHB", seg[1:6])
            if nf != 3:
                raise ValueError("jpeg: %d component(s): only three-component YCbCr files are supported (grey and CMYK are not)" % nf)
            frame = (width, height, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(3)])
        elif m == 0xC2:
            raise ValueError("jpeg: progressive files are not supported")
        elif m in (0xC1, 0xC3, 0xC5, 0xC6, 0xC7):
            raise ValueError("jpeg: only baseline (SOF0) files are supported, this one has SOF%d" % (m - 0xC0))
        elif 0xC9 <= m <= 0xCF and m != 0xCC:
            raise ValueError("jpeg: arithmetic coding is not supported")
        elif m == 0xCC:
            raise ValueError("jpeg: arithmetic coding is not supported")
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                counts = list(seg[k + 1:k + 17])
                n = sum(counts)
                (ac_tab if seg[k] >> 4 else dc_tab)[seg[k] & 15] = _huffman(counts, list(seg[k + 17:k + 17 + n]))
                k += 17 + n
        elif m == 0xDD:
            if struct.unpack(">H", seg[:2])[0]:
                raise ValueError("jpeg: restart intervals are not supported")
        elif m == 0xDA:
            if frame is None:
                raise ValueError("jpeg: SOS before SOF")
            if seg[0] != 3 or seg[7] != 0 or seg[8] != 63 or seg[9] != 0:
                raise ValueError("jpeg: one interleaved scan of all three components is expected")
            scan = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(3)]
            break
        else:
            raise ValueError("jpeg: marker FF%02X is not supported" % m)
    width, height, comps = frame
    if [c[0] for c in comps] != [s[0] for s in scan]:
        raise ValueError("jpeg: the scan's components are not the frame's")
    if (comps[0][1], comps[0][2]) not in LAYOUTS or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
        raise ValueError("jpeg: sampling factors %s are none of 4:4:4, 4:2:0, 4:2:2, 4:4:0" % [(c[1], c[2]) for c in comps])
    hmax, vmax = comps[0][1], comps[0][2]
    mx, my = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    coef = [np.zeros((my * c[2], mx * c[1], 64), np.int16) for c in comps]
    br, pred = _Bits(data, at), [0, 0, 0]
    for y in range(my):
        for x in range(mx):
            for i, c in enumerate(comps):
                dc, ac = dc_tab[scan[i][1]], ac_tab[scan[i][2]]
                for v in range(c[2]):
                    for h in range(c[1]):
                        blk = coef[i][y * c[2] + v, x * c[1] + h]
                        t = _symbol(br, dc)
                        pred[i] += _extend(br.bits(t), t)
                        blk[0] = pred[i]
                        k = 1
                        while k < 64:
                            rs = _symbol(br, ac)
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise ValueError("jpeg: a run past the block's end")
                            blk[ZIGZAG[k]] = _extend(br.bits(s), s)
                            k += 1
    if data[br.at:br.at + 2] != b"\xff\xd9":
        raise ValueError("jpeg: EOI expected behind the scan")
    return Parsed(width, height, [Component(c[0], c[1], c[2], qt[c[3]].copy(), coef[i].reshape(coef[i].shape[0], coef[i].shape[1], 8, 8)) for i, c in enumerate(comps)])


# ---------------------------------------------------------------- the float64 decoder

def _idct_matrix():
    """T.81 A.3.3: s[y][x] = 1/4 sum_u sum_v C(u) C(v) S[v][u] cos((2x+1) u pi / 16) cos((2y+1) v pi / 16), C(0) = 1/sqrt 2: s = A S A^T"""
    x, u = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    a = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    a[:, 0] *= np.sqrt(0.5)
    return a


def _plane(comp):
    """every block's 64 terms A[y, v] A[x, u] S[v][u] added in an order that does not tell (v, u) from (u, v) -- term (v, u) + term (u, v)
    first, then the 36 unordered pairs in a fixed order --, so that the decode of transposed data is the transposed decode to the bit"""
    a = _idct_matrix()
    basis = a[:, None, :, None] * a[None, :, None, :]                          # [y, x, v, u]
    f = comp.coef.astype(np.float64) * comp.table.astype(np.float64)
    t = basis[None, None] * f[:, :, None, None, :, :]                           # [by, bx, y, x, v, u]
    sym = t + t.swapaxes(-1, -2)
    iv, iu = np.triu_indices(8)
    s = (sym[..., iv, iu] * np.where(iv == iu, 0.5, 1.0)).sum(-1) + 128.0
    by, bx = s.shape[:2]
    return s.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _up2(a, axis):
    """centred siting, by two: out[2i] = 3/4 a[i] + 1/4 a[i-1], out[2i+1] = 3/4 a[i] + 1/4 a[i+1]; the array's border repeated"""
    a = np.moveaxis(a, axis, 0)
    before = np.concatenate([a[:1], a[:-1]])
    after = np.concatenate([a[1:], a[-1:]])
    out = np.empty((2 * a.shape[0],) + a.shape[1:], np.float64)
    out[0::2] = 0.75 * a + 0.25 * before
    out[1::2] = 0.75 * a + 0.25 * after
    return np.moveaxis(out, 0, axis)


def decode_f64(parsed, edge, clamp=False):
    """(rgb float64 [h, w, 3] unrounded, rgb u8, planes): planes = the three float64 planes Y, Cb, Cr ahead of upsampling and conversion,
    each over the whole-MCU block grid at its own resolution, level shift included.
    clamp: T.81 A.3.1 ends the inverse DCT by clamping every reconstructed sample to [0, 255], which an integer decoder does and a
    float pipeline that keeps going (a JPEG XL decoder) does not; the two differ only where a block overshoots.
    edge="libjpeg": a subsampled component ends at ceil(width / factor) x ceil(height / factor) and its last column and row are repeated
    beyond; edge="padded": it ends where the block grid padded to whole MCUs ends (what the blocks beyond the picture hold takes part)"""
    if edge not in ("libjpeg", "padded"):
        raise ValueError("edge=libjpeg|padded")
    w, h = parsed.width, parsed.height
    planes = [np.clip(_plane(c), 0.0, 255.0) if clamp else _plane(c) for c in parsed.components]
    full = []
    for c, p in zip(parsed.components, planes):
        fh, fv = parsed.hmax // c.h, parsed.vmax // c.v
        if edge == "libjpeg":
            p = p[:-(-h // fv), :-(-w // fh)]
        if fh == 2:
            p = _up2(p, 1)
        if fv == 2:
            p = _up2(p, 0)
        full.append(p[:h, :w])
    y, cb, cr = full[0], full[1] - 128.0, full[2] - 128.0
    kr, kb = 0.299, 0.114
    kg = 1.0 - kr - kb
    rgb = np.stack([y + 2 * (1 - kr) * cr,                                               # 1.402
                    y - 2 * (1 - kb) * kb / kg * cb - 2 * (1 - kr) * kr / kg * cr,       # 0.344136..., 0.714136...
                    y + 2 * (1 - kb) * cb], -1)                                           # 1.772
    u8 = np.clip(np.floor(rgb + 0.5), 0, 255).astype(np.uint8)
    return rgb, u8, planes


# ---------------------------------------------------------------- the dump tools/jxlsynth reads (jpegdata=PATH)

DUMP_MAGIC = 0x4447504A   # "JPGD"


def write_dump(parsed, path):
    """little-endian: int32 magic, width, height; per component Y, Cb, Cr: int32 h factor, v factor, blocks_x, blocks_y; per component
    64 x uint16 table [v][u]; per component blocks_y x blocks_x x 64 x int16 [by][bx][v][u] (v: vertical frequency)"""
    with open(path, "wb") as fp:
        fp.write(struct.pack("<3i", DUMP_MAGIC, parsed.width, parsed.height))
        for c in parsed.components:
            fp.write(struct.pack("<4i", c.h, c.v, c.coef.shape[1], c.coef.shape[0]))
        for c in parsed.components:
            fp.write(np.ascontiguousarray(c.table, "<u2").tobytes())
        for c in parsed.components:
            fp.write(np.ascontiguousarray(c.coef, "<i2").tobytes())


def transposed(parsed):
    """the same data with x and y exchanged: every block, the block grids and the tables transposed, the sampling factors swapped"""
    return Parsed(parsed.height, parsed.width, [Component(c.id, c.v, c.h, c.table.T.copy(), np.ascontiguousarray(c.coef.transpose(1, 0, 3, 2))) for c in parsed.components])


def fixture(name):
    """(the file's bytes, Pillow's decode of it u8 [h, w, 3])"""
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as fp:
        data = fp.read()
    return data, np.load(os.path.join(GOLDEN, name + ".rgb.npy"))


def dump_path(parsed, name):
    os.makedirs(CACHE, exist_ok=True)
    path = os.path.join(CACHE, "jpeg_%s.jpgd" % name)
    tmp = path + ".tmp%d" % os.getpid()
    write_dump(parsed, tmp)
    os.replace(tmp, path)
    return path


def transcoded(parsed, name, **opts):
    """the YCbCr VarDCT stream that carries `parsed` (build/jxlsynth vardct W H 1 OUT jpegdata=DUMP), cached by the dump's content"""
    dump = dump_path(parsed, name)
    with open(dump, "rb") as fp:
        key = hashlib.sha256(fp.read() + repr(sorted(opts.items())).encode()).hexdigest()[:16]
    path = os.path.join(CACHE, "jpeg_%s_%s.jxl" % (name, key))
    if not os.path.exists(path):
        tmp = path + ".tmp%d" % os.getpid()
        subprocess.run([SYNTH, "vardct", str(parsed.width), str(parsed.height), "1", tmp, "jpegdata=" + dump] + ["%s=%s" % kv for kv in sorted(opts.items())], check=True, stderr=subprocess.DEVNULL)
        os.replace(tmp, path)
    with open(path, "rb") as fp:
        return fp.read()
