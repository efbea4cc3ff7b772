"""The preview JPEG restated in numpy ("a preview's JPEG"): the file libjpeg writes for 8-bit planar 4:2:0
planes with its default (accurate integer) DCT, Annex K's tables scaled by a quality, and no restart markers.

Nothing here follows the kernels of handbrake_amd/csrc/jpeg.hip: the transform runs over whole arrays of blocks, the entropy
coder is one serial walk with libjpeg's own put-buffer, and the file is built front to back.  tests/test_preview_jpeg_cpu.py
holds it to Pillow (libjpeg-turbo) byte for byte; the GPU tests hold the encoder to it.
"""
import numpy as np

# ITU-T T.81 Annex K.1, natural (row-major) order
LUMA_BASE = [
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99]
CHROMA_BASE = [
    17, 18, 24, 47, 99, 99, 99, 99,
    18, 21, 26, 66, 99, 99, 99, 99,
    24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99]

# Annex K.3: (codes of each length 1 .. 16, the symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa])
HUFFMAN = {0x00: DC_LUMA, 0x10: AC_LUMA, 0x01: DC_CHROMA, 0x11: AC_CHROMA}      # by DHT class << 4 | id

HEADER_BYTES = 623


def _zigzag():
    order = sorted(range(64), key=lambda i: ((i // 8 + i % 8), (i // 8 if (i // 8 + i % 8) & 1 else i % 8)))
    return order


ZIGZAG = _zigzag()          # ZIGZAG[k]: natural index of the k-th coefficient of the scan


def quant_table(base, quality):
    """jpeg_quality_scaling and jpeg_add_quant_table (baseline): natural order"""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((b * s + 50) // 100, 1), 255) for b in base]


def code_table(spec):
    """symbol -> (code, length), the canonical assignment of Annex C"""
    bits, vals = spec
    assert sum(bits) == len(vals)
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


# ---------------------------------------------------------------- the file's segments
def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def dqt_segment(index, table):
    return _segment(0xDB, [index] + [table[n] for n in ZIGZAG])


def dht_segment(tc_th):
    bits, vals = HUFFMAN[tc_th]
    return _segment(0xC4, [tc_th] + bits + vals)


def header(width, height, quality):
    out = b"\xff\xd8"
    out += _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += dqt_segment(0, quant_table(LUMA_BASE, quality)) + dqt_segment(1, quant_table(CHROMA_BASE, quality))
    out += _segment(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") +
                    bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for t in (0x00, 0x10, 0x01, 0x11):
        out += dht_segment(t)
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == HEADER_BYTES
    return out


# ---------------------------------------------------------------- blocks
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first):
    """one pass of jfdctint.c's jpeg_fdct_islow over the LAST axis of d (int64 [..., 8])"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = 13 - 2 if first else 13 + 2
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2] = _descale(z1 + t13 * 6270, n)
    out[..., 6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def forward_dct(blocks):
    """blocks: int [n, 8, 8] of level-shifted samples -> 8 x the DCT, rows first and then columns"""
    rows = _pass(blocks.astype(np.int64), True)
    return _pass(rows.transpose(0, 2, 1), False).transpose(0, 2, 1)


def quantize(coefs, table):
    """coefs int [n, 8, 8]; table natural order: |c| + (d >> 1) over d = q << 3, truncating, the sign put back"""
    d = (np.asarray(table, np.int64) << 3).reshape(8, 8)
    mag = (np.abs(coefs) + (d >> 1)) // d
    return np.where(coefs < 0, -mag, mag)


def plane_blocks(plane, bw, bh, table):
    """the quantised blocks [bh, bw, 64] (natural order) of a plane padded to bw x bh blocks by its last column and row"""
    h, w = plane.shape
    p = np.pad(plane.astype(np.int64), ((0, bh * 8 - h), (0, bw * 8 - w)), mode="edge") - 128
    blocks = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(bh * bw, 8, 8)
    return quantize(forward_dct(blocks), table).reshape(bh, bw, 64)


def scan_blocks(planes, quality):
    """Every block of the scan in coding order: a list of (component, coefficients in ZIGZAG order or None for a dummy).
    A dummy is a luma block of an MCU that lies wholly outside the ceil(w / 8) x ceil(h / 8) real blocks."""
    y, cb, cr = planes
    h, w = y.shape
    assert w % 2 == 0 and h % 2 == 0 and cb.shape == cr.shape == (h // 2, w // 2)
    mw, mh = -(-w // 16), -(-h // 16)
    qy, qc = quant_table(LUMA_BASE, quality), quant_table(CHROMA_BASE, quality)
    yb = plane_blocks(y, 2 * mw, 2 * mh, qy)[:, :, ZIGZAG]
    cbb = plane_blocks(cb, mw, mh, qc)[:, :, ZIGZAG]
    crb = plane_blocks(cr, mw, mh, qc)[:, :, ZIGZAG]
    real_w, real_h = -(-w // 8), -(-h // 8)
    out = []
    for my in range(mh):
        for mx in range(mw):
            for by, bx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                yy, xx = 2 * my + by, 2 * mx + bx
                out.append((0, yb[yy, xx] if yy < real_h and xx < real_w else None))
            out.append((1, cbb[my, mx]))
            out.append((2, crb[my, mx]))
    return out


def _magnitude(v):
    """(category, the value's low bits: v, or v - 1 for a negative one)"""
    n = int(abs(v)).bit_length()
    return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)


def block_symbols(zz, pred, dc_table, ac_table):
    """one block as a list of (bits, length) and its DC; zz None: a dummy block - DC difference 0 and end of block"""
    if zz is None:
        return [dc_table[0], ac_table[0x00]], pred
    out = []
    n, low = _magnitude(int(zz[0]) - pred)
    out.append(dc_table[n])
    if n:
        out.append((low, n))
    run = 0
    for k in range(1, 64):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(ac_table[0xF0])
            run -= 16
        n, low = _magnitude(v)
        out.append(ac_table[(run << 4) | n])
        out.append((low, n))
        run = 0
    if run:
        out.append(ac_table[0x00])
    return out, int(zz[0])


def bit_string(symbols):
    return "".join(format(b, "0%db" % n) for b, n in symbols)


def coded_blocks(planes, quality):
    """[(component, dummy, coefficients in scan order (zeros and the inherited DC for a dummy), bit string)] in coding order"""
    tables = {t: code_table(HUFFMAN[t]) for t in HUFFMAN}
    pred = [0, 0, 0]
    out = []
    for comp, zz in scan_blocks(planes, quality):
        t = 0 if comp == 0 else 1
        sym, dc = block_symbols(zz, pred[comp], tables[0x00 | t], tables[0x10 | t])
        pred[comp] = dc
        coefs = [dc] + [0] * 63 if zz is None else [int(v) for v in zz]
        out.append((comp, zz is None, coefs, bit_string(sym)))
    return out


def entropy_segment(planes, quality):
    """the scan's bytes: the blocks' bits, the last byte filled with ones, a zero byte behind every 0xFF"""
    bits = "".join(b[3] for b in coded_blocks(planes, quality))
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""
    return raw.replace(b"\xff", b"\xff\x00")


def encode(planes, quality=90):
    """the whole file for (Y, Cb, Cr) uint8 planes of an even-sized 4:2:0 picture"""
    h, w = planes[0].shape
    return header(w, h, quality) + entropy_segment(planes, quality) + b"\xff\xd9"


# ---------------------------------------------------------------- reading a file's segments back (for the table tests)
def segments(data):
    """[(marker, payload)] up to and including SOS"""
    assert data[:2] == b"\xff\xd8"
    out, at = [], 2
    while True:
        assert data[at] == 0xFF
        marker, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        out.append((marker, bytes(data[at + 4:at + 2 + n])))
        at += 2 + n
        if marker == 0xDA:
            return out, at


# ---------------------------------------------------------------- contents (integer formulas: the same on every numpy)
def _hash(y, x, salt):
    v = (x.astype(np.uint64) * np.uint64(2654435761) + y.astype(np.uint64) * np.uint64(40503) + np.uint64(salt * 977 + 12345))
    v ^= v >> np.uint64(13)
    v = (v * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(16)
    return v


def _grid(h, w):
    return np.mgrid[0:h, 0:w]


def content(name, width, height):
    """(Y, Cb, Cr) uint8 planes of a 4:2:0 picture of the named content"""
    sizes = ((height, width), (height // 2, width // 2), (height // 2, width // 2))
    planes = []
    for c, (h, w) in enumerate(sizes):
        y, x = _grid(h, w)
        if name == "flat":
            p = np.full((h, w), (90, 120, 140)[c])
        elif name == "smooth":
            p = (3 * x + 2 * y + 40 * c) // 4 % 256
        elif name == "noise":
            p = (_hash(y, x, c) >> np.uint64(8)) & np.uint64(0xFF)
        elif name == "sat":
            p = np.where((_hash(y // 3, x // 5, c + 7) >> np.uint64(11)) & np.uint64(1), 255, 0)
        elif name == "sparse":
            # one (7, 7) cosine per block: the last coefficient of the scan behind 62 zeros
            amp = 20 + 10 * (((x // 8) + (y // 8) + c) % 7)
            table = np.round(np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16) * 1024).astype(np.int64)
            p = 128 + (amp * table[x % 8] * table[y % 8]) // (1 << 20)
        elif name == "formula":
            p = (x * x // 7 + y * 3 + ((x ^ y) & 31) * 3 + (_hash(y // 2, x // 2, c) & np.uint64(15)).astype(np.int64) + 50 * c) % 256
        else:
            raise KeyError(name)
        planes.append(np.clip(np.asarray(p, dtype=np.int64), 0, 255).astype(np.uint8))
    return tuple(planes)


CONTENTS = ("flat", "smooth", "noise", "sat", "sparse")
SIZES = ((8, 8), (16, 16), (24, 18), (18, 24), (34, 10), (48, 32), (130, 70), (640, 360))
QUALITIES_EXTRA = (1, 25, 50, 100)
QUALITY_SIZES = ((24, 18), (130, 70))
BIG = (1920, 1080)


def cases():
    """every (width, height, content, quality) of the tests, and the key of its golden entry"""
    out = []
    for (w, h) in SIZES:
        for q in (90,) + (QUALITIES_EXTRA if (w, h) in QUALITY_SIZES else ()):
            for c in CONTENTS:
                out.append((w, h, c, q))
    return out


def key(w, h, content_name, q):
    return "%dx%d_%s_q%d" % (w, h, content_name, q)


GOLDEN_BYTES_MAX = (48, 32)         # up to this size the golden file holds the file itself, beyond it length and SHA-256


def pillow_encode(planes, quality):
    """The reference: what Pillow (libjpeg-turbo, default DCT) writes for these planes.  Pillow takes no planar 4:2:0, so
    every chroma sample is repeated 2 x 2; libjpeg's h2v2 down-sampler gives each back exactly."""
    import io
    from PIL import Image
    y, cb, cr = planes
    h, w = y.shape
    full = [y] + [np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)[:h, :w] for p in (cb, cr)]
    im = Image.merge("YCbCr", [Image.fromarray(np.ascontiguousarray(p)) for p in full])
    out = io.BytesIO()
    im.save(out, "JPEG", quality=quality, subsampling=2)
    return out.getvalue()
