"""numpy restatement of the baseline JPEG decoder (pg_jpeg_*): header parse, Huffman decode, dequantisation, libjpeg's accurate integer
inverse DCT, libjpeg-turbo's "fancy" chroma upsampling and the YCbCr -> RGB conversion, written from the formulas and not from the
HIP / C++ sources.  It is held against Pillow's pixels (tests/test_jpegref_cpu.py), and the host stage and the kernels against it.

`mistakes`: a set of names of planted mistakes; each one must make the restatement differ from Pillow somewhere (the test names where):
  bias_swap    the 4:2:0 rounding biases 7 and 8 exchanged
  filter_at_2  the upsampling filter applied at a chroma width of 2 (libjpeg replicates there)
  pass_swap    rows first (shift 11), then columns (shift 18)
  no_32768     the rounding term missing in the blue channel
  zigzag_T     the zigzag order transposed
  no_dc_reset  the DC predictors kept across a restart marker
  pad_bottom   the row below the last real chroma row taken from the block padding instead of replicated
"""
import numpy as np

REASONS = ("ok", "not_jpeg", "progressive", "lossless", "hierarchical", "arithmetic", "precision", "components", "colorspace",
           "sampling", "multiscan", "dnl", "size", "malformed")


class Refused(Exception):
    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


class EntropyError(Exception):
    pass


def _zigzag():
    """Zigzag position -> (row, col): walk the anti-diagonals, alternating direction."""
    order = []
    for s in range(15):
        cells = [(r, s - r) for r in range(8) if 0 <= s - r < 8]
        order += cells if s % 2 else cells[::-1]
    return order


ZIGZAG = _zigzag()
NATURAL = np.array([r * 8 + c for r, c in ZIGZAG])
NATURAL_T = np.array([c * 8 + r for r, c in ZIGZAG])


def _u16(d, p):
    return (d[p] << 8) | d[p + 1]


def parse(data):
    """Header up to SOS -> dict, or Refused(reason)."""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Refused("not_jpeg")
    h = dict(qt={}, dc={}, ac={}, ri=0, jfif=False, adobe=None, sof=False)
    pos = 2
    while True:
        if pos >= n or d[pos] != 0xFF:
            raise Refused("malformed")
        while pos < n and d[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise Refused("malformed")
        m = d[pos]
        pos += 1
        if m in (0, 1) or 0xD0 <= m <= 0xD9 or pos + 2 > n:
            raise Refused("malformed")
        ln = _u16(d, pos)
        if ln < 2 or ln > n - pos:
            raise Refused("malformed")
        seg = d[pos + 2:pos + ln]
        pos += ln
        if m == 0xE0:
            h["jfif"] |= len(seg) >= 14 and seg[:5] == b"JFIF\0"
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                h["adobe"] = seg[11]
        elif m == 0xDB:
            while seg:
                pq, tq = seg[0] >> 4, seg[0] & 15
                need = 1 + 64 * (1 + pq)
                if tq > 3 or pq > 1 or len(seg) < need:
                    raise Refused("malformed")
                vals = [(_u16(seg, 1 + 2 * i) if pq else seg[1 + i]) for i in range(64)]
                h["qt"][tq] = vals                                  # zigzag order, as in the file
                seg = seg[need:]
        elif m == 0xC4:
            while seg:
                tc, th = seg[0] >> 4, seg[0] & 15
                if tc > 1 or th > 3 or len(seg) < 17:
                    raise Refused("malformed")
                counts = list(seg[1:17])
                tot = sum(counts)
                if tot > 256 or len(seg) < 17 + tot:
                    raise Refused("malformed")
                h["ac" if tc else "dc"][th] = (counts, list(seg[17:17 + tot]))
                seg = seg[17 + tot:]
        elif m in (0xC0, 0xC1):
            if h["sof"] or len(seg) < 6:
                raise Refused("malformed")
            h["sof"] = True
            h["height"], h["width"], nc = _u16(seg, 1), _u16(seg, 3), seg[5]
            if seg[0] != 8:
                raise Refused("precision")
            if len(seg) != 6 + 3 * nc:
                raise Refused("malformed")
            if nc not in (1, 3):
                raise Refused("components")
            if not (1 <= h["height"] <= 16384 and 1 <= h["width"] <= 16384):
                raise Refused("size")
            h["comps"] = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)]
            if any(not (1 <= ch <= 4 and 1 <= cv <= 4 and tq <= 3) for _, ch, cv, tq in h["comps"]):
                raise Refused("malformed")
        elif m == 0xC2:
            raise Refused("progressive")
        elif m == 0xC3:
            raise Refused("lossless")
        elif m in (0xC5, 0xC6, 0xC7, 0xDE, 0xDF):
            raise Refused("hierarchical")
        elif 0xC9 <= m <= 0xCF:
            raise Refused("arithmetic")
        elif m == 0xC8:
            raise Refused("malformed")
        elif m == 0xDC:
            raise Refused("dnl")
        elif m == 0xDD:
            if len(seg) != 2:
                raise Refused("malformed")
            h["ri"] = _u16(seg, 0)
        elif m == 0xDA:
            if not h["sof"] or len(seg) < 1 or not (1 <= seg[0] <= 4) or len(seg) != 4 + 2 * seg[0]:
                raise Refused("malformed")
            comps = h["comps"]
            if seg[0] != len(comps):
                raise Refused("multiscan")
            h["tabs"] = []
            for c, (cid, _, _, tq) in enumerate(comps):
                td, ta = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
                if seg[1 + 2 * c] != cid or td not in h["dc"] or ta not in h["ac"] or tq not in h["qt"]:
                    raise Refused("malformed")
                h["tabs"].append((td, ta))
            if len(comps) == 1:
                h["hs"] = h["vs"] = 1
            else:
                if not h["jfif"]:
                    if h["adobe"] is not None:
                        if h["adobe"] != 1:
                            raise Refused("colorspace")
                    elif bytes(c[0] for c in comps) == b"RGB":
                        raise Refused("colorspace")
                h["hs"], h["vs"] = comps[0][1], comps[0][2]
                if (h["hs"], h["vs"]) not in ((1, 1), (2, 1), (2, 2)) or any(c[1:3] != (1, 1) for c in comps[1:]):
                    raise Refused("sampling")
            h["ncomp"] = len(comps)
            h["scan"] = pos
            return h


def block_grid(height, width, ncomp, hs, vs):
    mx, my = -(-width // (8 * hs)), -(-height // (8 * vs))
    return [(mx * hs, my * vs)] + [(mx, my)] * (ncomp - 1)             # (bw, bh) per component


def quant_natural(h, mistakes=()):
    """(4, 64) uint16, natural order; tables the file does not define are zero."""
    nat = NATURAL_T if "zigzag_T" in mistakes else NATURAL
    out = np.zeros((4, 64), dtype=np.uint16)
    for tq, vals in h["qt"].items():
        out[tq, nat] = vals
    return out


def _codes(spec):
    counts, vals = spec
    table, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            table[(l, code)] = vals[k]
            code += 1
            k += 1
        if code >= (1 << l) and counts[l - 1]:
            raise EntropyError("bad Huffman table")
        code <<= 1
    return table


def _segments(d, pos):
    """The scan from `pos`: [(bits as a '0'/'1' string, marker that ended it)], stuffing undone."""
    segs, cur, n = [], bytearray(), len(d)
    while True:
        if pos >= n:
            segs.append((cur, None))
            return segs
        b = d[pos]
        if b != 0xFF:
            cur.append(b)
            pos += 1
            continue
        if pos + 1 >= n:
            segs.append((cur, None))
            return segs
        if d[pos + 1] == 0:
            cur.append(0xFF)
            pos += 2
            continue
        while pos + 1 < n and d[pos + 1] == 0xFF:
            pos += 1
        if pos + 1 >= n:
            segs.append((cur, None))
            return segs
        segs.append((cur, d[pos + 1]))
        if not (0xD0 <= d[pos + 1] <= 0xD7):
            return segs
        cur = bytearray()
        pos += 2


class _Reader:
    def __init__(self, seg):
        self.s = "".join(f"{b:08b}" for b in seg)
        self.p = 0

    def symbol(self, table):
        for l in range(1, 17):
            if self.p + l > len(self.s):
                raise EntropyError("data ends inside an MCU")
            v = table.get((l, int(self.s[self.p:self.p + l], 2)))
            if v is not None:
                self.p += l
                return v
        raise EntropyError("no such Huffman code")

    def value(self, s):
        if s == 0:
            return 0
        if self.p + s > len(self.s):
            raise EntropyError("data ends inside an MCU")
        v = int(self.s[self.p:self.p + s], 2)
        self.p += s
        return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def entropy_decode(data, h=None, mistakes=()):
    """-> list per component of (bh * bw, 64) int16: the padded block grid in raster order, blocks in natural order."""
    d = bytes(data)
    h = h or parse(d)
    nat = NATURAL_T if "zigzag_T" in mistakes else NATURAL
    grid = block_grid(h["height"], h["width"], h["ncomp"], h["hs"], h["vs"])
    coef = [np.zeros((bw * bh, 64), dtype=np.int16) for bw, bh in grid]
    dct = [_codes(h["dc"][td]) for td, _ in h["tabs"]]
    act = [_codes(h["ac"][ta]) for _, ta in h["tabs"]]
    samp = [(h["hs"], h["vs"])] + [(1, 1)] * (h["ncomp"] - 1)
    segs = _segments(d, h["scan"])
    si, rd = 0, _Reader(segs[0][0])
    pred = [0] * h["ncomp"]
    mcux, mcuy = grid[0][0] // h["hs"], grid[0][1] // h["vs"]
    for m in range(mcux * mcuy):
        my, mx = divmod(m, mcux)
        if h["ri"] and m and m % h["ri"] == 0:
            if segs[si][1] != 0xD0 + (si & 7) or len(rd.s) - rd.p >= 8 or si + 1 >= len(segs):
                raise EntropyError("RSTn missing or out of sequence")
            si += 1
            rd = _Reader(segs[si][0])
            if "no_dc_reset" not in mistakes:
                pred = [0] * h["ncomp"]
        for c in range(h["ncomp"]):
            for v in range(samp[c][1]):
                for u in range(samp[c][0]):
                    blk = coef[c][(my * samp[c][1] + v) * grid[c][0] + mx * samp[c][0] + u]
                    s = rd.symbol(dct[c])
                    if s > 15:
                        raise EntropyError("DC category")
                    pred[c] += rd.value(s)
                    blk[0] = np.int16(((pred[c] + 32768) & 0xffff) - 32768)
                    k = 1
                    while k < 64:
                        rs = rd.symbol(act[c])
                        r, s = rs >> 4, rs & 15
                        if s:
                            k += r
                            if k > 63:
                                raise EntropyError("coefficient index past 63")
                            blk[nat[k]] = rd.value(s)
                            k += 1
                        elif r == 15:
                            k += 16
                            if k > 64:
                                raise EntropyError("coefficient index past 63")
                        else:
                            break
    if segs[si][1] != 0xD9 or len(rd.s) - rd.p >= 8:
        raise EntropyError("no EOI behind the last MCU")
    return coef


def _idct8(x, s):
    """x: (..., 8) int32, along the last axis; 32-bit wrap-around."""
    x = [x[..., k].astype(np.int32) for k in range(8)]
    i32 = np.int32
    z1 = (x[2] + x[6]) * i32(4433)
    t2 = z1 - x[6] * i32(15137)
    t3 = z1 + x[2] * i32(6270)
    t0 = (x[0] + x[4]) << i32(13)
    t1 = (x[0] - x[4]) << i32(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a, b, c, d = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = a + d, b + c, a + c, b + d
    z5 = (z3 + z4) * i32(9633)
    a, b, c, d = a * i32(2446), b * i32(16819), c * i32(25172), d * i32(12299)
    z1, z2 = z1 * i32(-7373), z2 * i32(-20995)
    z3, z4 = z3 * i32(-16069) + z5, z4 * i32(-3196) + z5
    a, b, c, d = a + z1 + z3, b + z2 + z4, c + z2 + z3, d + z1 + z4
    y = [t10 + d, t11 + c, t12 + b, t13 + a, t13 - a, t12 - b, t11 - c, t10 - d]
    r = i32(1 << (s - 1))
    return np.stack([(v + r) >> i32(s) for v in y], axis=-1)


def idct_blocks(coef, q, mistakes=()):
    """coef (nb, 64) int16, q (64,) uint16, natural order -> (nb, 8, 8) uint8 samples."""
    with np.errstate(over="ignore"):
        blk = (coef.astype(np.int32) * q.astype(np.int32)[None, :]).reshape(-1, 8, 8)       # [row, col]
        if "pass_swap" in mistakes:
            ws = _idct8(blk, 11)
            out = _idct8(ws.transpose(0, 2, 1), 18).transpose(0, 2, 1)
        else:
            ws = _idct8(blk.transpose(0, 2, 1), 11).transpose(0, 2, 1)                      # columns: x_k = row k of the column
            out = _idct8(ws, 18)                                                            # rows
    s = ((out & 1023) ^ 512) - 512
    return np.clip(s + 128, 0, 255).astype(np.uint8)


def plane_from_blocks(samples, bw, bh):
    return samples.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _shift(p, d, axis):
    """p shifted by d along axis with the edge replicated: out[i] = p[clamp(i + d)]."""
    idx = np.clip(np.arange(p.shape[axis]) + d, 0, p.shape[axis] - 1)
    return np.take(p, idx, axis=axis)


def upsample(plane, cw, ch, hs, vs, mistakes=()):
    """The padded chroma plane -> (ch * vs, cw * hs) int32 at full resolution, over the REAL plane (ch x cw)."""
    p = plane[:ch, :cw].astype(np.int32)
    if hs == 1:
        return p
    if cw <= 2 and "filter_at_2" not in mistakes:
        return np.repeat(np.repeat(p, vs, axis=0), 2, axis=1)
    if vs == 1:
        even = (3 * p + _shift(p, -1, 1) + 1) >> 2
        odd = (3 * p + _shift(p, 1, 1) + 2) >> 2
        return np.stack([even, odd], axis=2).reshape(ch, 2 * cw)
    up, dn = _shift(p, -1, 0), _shift(p, 1, 0)
    if "pad_bottom" in mistakes and plane.shape[0] > ch:
        dn = dn.copy()
        dn[-1] = plane[ch, :cw]
    be, bo = (7, 8) if "bias_swap" in mistakes else (8, 7)
    rows = []
    for t in (3 * p + up, 3 * p + dn):
        even = (3 * t + _shift(t, -1, 1) + be) >> 4
        odd = (3 * t + _shift(t, 1, 1) + bo) >> 4
        rows.append(np.stack([even, odd], axis=2).reshape(ch, 2 * cw))
    return np.stack(rows, axis=1).reshape(2 * ch, 2 * cw)


def colour(Y, cb, cr, mistakes=()):
    Y, cb, cr = Y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    B = Y + ((116130 * cb + (0 if "no_32768" in mistakes else 32768)) >> 16)
    return np.clip(np.stack([R, G, B], axis=-1), 0, 255).astype(np.uint8)


def pixels_from_coefficients(coef, qt, qsel, height, width, ncomp, hs, vs, mistakes=()):
    """coef: per component (bh * bw, 64) int16; qt (4, 64); qsel: table per component -> (height, width, 3) uint8."""
    grid = block_grid(height, width, ncomp, hs, vs)
    planes = [plane_from_blocks(idct_blocks(coef[c], qt[qsel[c]], mistakes), *grid[c]) for c in range(ncomp)]
    Y = planes[0][:height, :width]
    if ncomp == 1:
        return np.repeat(Y[:, :, None], 3, axis=2)
    cw, ch = -(-width // hs), -(-height // vs)
    cb = upsample(planes[1], cw, ch, hs, vs, mistakes)[:height, :width]
    cr = upsample(planes[2], cw, ch, hs, vs, mistakes)[:height, :width]
    return colour(Y, cb, cr, mistakes)


def decode(data, mistakes=()):
    """File bytes -> (H, W, 3) uint8, what Pillow gives for Image.open(f).convert('RGB')."""
    h = parse(data)
    coef = entropy_decode(data, h, mistakes)
    return pixels_from_coefficients(coef, quant_natural(h, mistakes), [c[3] for c in h["comps"]], h["height"], h["width"], h["ncomp"],
                                    h["hs"], h["vs"], mistakes)


def layout(shapes):
    """The buffers' layout for images [(height, width, ncomp, hs, vs)] (ncomp 0 = supplied by the caller): per image (coef_off[3],
    plane_off[3], grid), and (coef_bytes, workspace_bytes)."""
    up = lambda v, a: -(-v // a) * a
    coef, ws, out = up(len(shapes) * 640, 128), 0, []
    for height, width, ncomp, hs, vs in shapes:
        co, po, grid = [0, 0, 0], [0, 0, 0], []
        if ncomp:
            grid = block_grid(height, width, ncomp, hs, vs)
            for c, (bw, bh) in enumerate(grid):
                co[c], coef = coef, coef + bw * bh * 128
                ws = up(ws, 256)
                po[c], ws = ws, ws + bw * bh * 64
        out.append((co, po, grid))
    return out, (coef, up(ws, 256))


def first_mismatch(a, b):
    """None, or 'y=.. x=.. channel=.. (got .., want ..)' of the first differing sample."""
    if a.shape != b.shape:
        return f"shape {a.shape} != {b.shape}"
    bad = np.argwhere(a != b)
    if not len(bad):
        return None
    y, x, c = bad[0]
    return f"y={y} x={x} channel={'RGB'[c]} (got {a[y, x, c]}, want {b[y, x, c]})"
