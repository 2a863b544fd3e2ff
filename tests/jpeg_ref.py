"""The JPEG encoder of DESIGN.md 3.12 restated in numpy (int64 throughout), from the stated integer rule and ITU-T T.81: the reference
yk_jpeg_encode_ragged_u8 has to equal bit for bit.  encode() returns the entropy-coded scan (byte-stuffed, padded with 1-bits) and
statistics about the paths it took; file() wraps it with jpeg.assemble."""
import numpy as np

from k210_yolo_framework_amd import jpeg

T = jpeg.dct_table().astype(np.int64)
_DC = [jpeg.huffman_codes(jpeg.DC_LUMA_BITS, jpeg.DC_LUMA_VALS), jpeg.huffman_codes(jpeg.DC_CHROMA_BITS, jpeg.DC_CHROMA_VALS)]
_AC = [jpeg.huffman_codes(jpeg.AC_LUMA_BITS, jpeg.AC_LUMA_VALS), jpeg.huffman_codes(jpeg.AC_CHROMA_BITS, jpeg.AC_CHROMA_VALS)]


def planes(img):
    """[h, w, 3] uint8 -> (Y [16*my, 16*mx], Cb, Cr [8*my, 8*mx]) int64: edge replication on the RGB indices, colour, chroma average."""
    h, w = img.shape[:2]
    H, W = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    ys, xs = np.minimum(np.arange(H), h - 1), np.minimum(np.arange(W), w - 1)
    p = img[ys][:, xs].astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = np.clip((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, 0, 255)
    cb = np.clip(((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128, 0, 255)
    cr = np.clip(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128, 0, 255)
    sub = lambda c: (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    return y, sub(cb), sub(cr)


def block_coefficients(plane, qtab):
    """plane [8a, 8b] -> quantised coefficients [a, b, 64] in natural order, AC clamped to +-1023 (the DC is left for the difference)."""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    s = plane.reshape(a, 8, b, 8).transpose(0, 2, 1, 3) - 128               # [a, b, y, x]
    r = np.einsum('ux,abyx->abyu', T, s)
    assert np.abs(r).max(initial=0) < 2 ** 22
    r1 = (r + 512) >> 10
    assert np.abs(r1).max(initial=0) <= 4018
    c = np.einsum('vy,abyu->abvu', T, r1)                                   # the coefficient times 2^16
    assert np.abs(c).max(initial=0) < 1.3e8
    d = np.asarray(qtab, np.int64).reshape(8, 8)
    q = np.sign(c) * ((np.abs(c) + d * 32768) // (d * 65536))
    q = q.reshape(a, b, 64)
    clamped = int((np.abs(q[..., 1:]) > 1023).sum())
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    return q, clamped


def _size(v):
    return int(abs(int(v))).bit_length()


class _Bits:
    """MSB-first bit packer: whole bytes go to `out`, `total` counts every bit put."""

    def __init__(self):
        self.acc, self.n, self.total, self.out = 0, 0, 0, bytearray()

    def put(self, code, length):
        assert length > 0 and 0 <= code < (1 << length)
        self.acc = (self.acc << length) | code
        self.n += length
        self.total += length
        while self.n >= 8:
            self.n -= 8
            self.out.append(self.acc >> self.n)
            self.acc &= (1 << self.n) - 1


def encode(img, quality=75):
    """-> (scan bytes, stats).  stats: bits (before padding), stuffed, zrl, eob_only (blocks that are a DC code and EOB), clamped_ac,
    clamped_dc, blocks, and what stuffing_positions says of the unstuffed stream."""
    img = np.asarray(img)
    assert img.ndim == 3 and img.shape[2] == 3 and img.dtype == np.uint8 and img.shape[0] > 0 and img.shape[1] > 0
    qt = jpeg.quant_tables(quality).astype(np.int64)
    y, cb, cr = planes(img)
    qy, c0 = block_coefficients(y, qt[0])
    qb, c1 = block_coefficients(cb, qt[1])
    qr, c2 = block_coefficients(cr, qt[1])
    zz = jpeg.ZIGZAG
    st = dict(zrl=0, eob_only=0, clamped_ac=c0 + c1 + c2, clamped_dc=0, blocks=0)
    bits = _Bits()
    pred = [0, 0, 0]
    for my in range(cb.shape[0] // 8):
        for mx in range(cb.shape[1] // 8):
            blocks = [(0, qy[2 * my, 2 * mx]), (0, qy[2 * my, 2 * mx + 1]), (0, qy[2 * my + 1, 2 * mx]), (0, qy[2 * my + 1, 2 * mx + 1]),
                      (1, qb[my, mx]), (2, qr[my, mx])]
            for comp, blk in blocks:
                tab = 0 if comp == 0 else 1
                z = blk[zz]
                diff = int(z[0]) - pred[comp]
                pred[comp] = int(z[0])
                if abs(diff) > 2047:
                    st['clamped_dc'] += 1
                    diff = max(-2047, min(2047, diff))
                st['blocks'] += 1
                s = _size(diff)
                bits.put(int(_DC[tab][0][s]), int(_DC[tab][1][s]))
                if s:
                    bits.put(diff if diff >= 0 else diff - 1 + (1 << s), s)
                code, length = _AC[tab]
                run, emitted = 0, 0
                for k in range(1, 64):
                    v = int(z[k])
                    if v == 0:
                        run += 1
                        continue
                    while run >= 16:
                        bits.put(int(code[0xF0]), int(length[0xF0]))
                        st['zrl'] += 1
                        run -= 16
                    s = _size(v)
                    sym = run << 4 | s
                    bits.put(int(code[sym]), int(length[sym]))
                    bits.put(v if v >= 0 else v - 1 + (1 << s), s)
                    run, emitted = 0, emitted + 1
                if run:
                    bits.put(int(code[0]), int(length[0]))
                    if emitted == 0:
                        st['eob_only'] += 1
    st['bits'] = bits.total
    if bits.n:
        pad = 8 - bits.n
        bits.put((1 << pad) - 1, pad)
        bits.total -= pad
    raw = bytes(bits.out)
    st['stuffed'] = raw.count(b'\xff')
    st.update(stuffing_positions(raw))
    return raw.replace(b'\xff', b'\xff\x00'), st


CHUNK_BYTES, LANE_BYTES = 1248, 20          # the device stuffs a picture in chunks of 1248 unstuffed bytes, 63 lanes of 20 bytes each


def stuffing_positions(raw):
    """Where the 0xFF bytes of an unstuffed, padded stream lie in the device's chunks and lanes: unstuffed_bytes, ff_positions (int64,
    ascending), ff_at_lane_end (a lane's last byte), ff_at_chunk_end (a chunk's last byte: its 0x00 opens the next chunk's output),
    last_byte_ff (the picture's last byte, after the 1-padding)."""
    ff = np.flatnonzero(np.frombuffer(raw, np.uint8) == 0xFF).astype(np.int64)
    in_chunk = ff % CHUNK_BYTES
    return dict(unstuffed_bytes=len(raw), ff_positions=ff, ff_at_lane_end=int((in_chunk % LANE_BYTES == LANE_BYTES - 1).sum()),
                ff_at_chunk_end=int((in_chunk == CHUNK_BYTES - 1).sum()), last_byte_ff=bool(len(raw)) and raw[-1] == 0xFF)


def file(img, quality=75):
    """The complete JFIF file of a picture."""
    scan, _ = encode(img, quality)
    return jpeg.assemble(img.shape[0], img.shape[1], jpeg.quant_tables(quality), scan)


# ---- the pictures the CPU and the GPU tests share -----------------------------------------------------------------------------------
SIZES = [(1, 1), (8, 8), (16, 16), (17, 9), (9, 17), (15, 33), (7, 640), (640, 7), (96, 128)]
QUALITIES = (1, 75, 100)
NOISE_SEED = 5


def picture(kind, h, w, seed=NOISE_SEED):
    """noise | flat | ramp (horizontal) | checker (saturated red / blue, 3-pixel cells: chroma extremes inside every block) |
    bw (black / white 16-pixel cells: the largest DC differences)."""
    if kind == 'noise':
        return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'flat':
        return np.full((h, w, 3), (h * 7 + w * 3) % 256, np.uint8)
    if kind == 'ramp':
        row = (np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)
        return np.ascontiguousarray(np.broadcast_to(row[None, :, None], (h, w, 3)))
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'checker':
        red = ((yy // 3 + xx // 3) % 2 == 0)[..., None]
        return np.where(red, np.array([255, 0, 0], np.uint8), np.array([0, 0, 255], np.uint8)).astype(np.uint8)
    if kind == 'bw':
        return np.ascontiguousarray(np.broadcast_to((((yy // 16 + xx // 16) % 2) * 255).astype(np.uint8)[..., None], (h, w, 3)))
    raise ValueError(kind)


KINDS = ('noise', 'flat', 'ramp', 'checker', 'bw')


def batch_pictures(n=33):
    """n pictures cycling through SIZES and KINDS (9 and 5 are coprime: 33 pictures hold 33 different pairs; the first is 96 x 128 noise)."""
    out = []
    for i in range(n):
        h, w = SIZES[(8 + i) % len(SIZES)]
        out.append(picture(KINDS[i % len(KINDS)], h, w))
    return out


_cache = {}


def encode_cached(i, quality, n=33):
    """encode(batch_pictures(n)[i], quality), computed once per session."""
    key = (i, quality, n)
    if key not in _cache:
        _cache[key] = encode(batch_pictures(n)[i], quality)
    return _cache[key]
