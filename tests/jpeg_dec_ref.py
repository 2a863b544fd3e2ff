"""The JPEG decoder of DESIGN.md 3.12 restated in numpy / plain Python: a sequential T.81 F.2.2 Huffman decode, then the stated integer
rule (dequantise, clamp, IDCT columns then rows, triangle upsampling, 16-bit colour).  Starts from jpeg.parse_baseline's output and shares
no code with the kernels: yk_jpeg_decode_ragged_u8 has to equal decode() byte for byte, whatever its chunk size."""
import io
import re

import numpy as np

from k210_yolo_framework_amd import jpeg

T = jpeg.idct_table().astype(np.int64)


def _lut(bits, vals):
    """T.81 Annex C codes as a table over the next 16 bits: length << 8 | symbol, 0 where no code matches."""
    lut = np.zeros(65536, np.int64)
    code, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            lut[code << (16 - ln):(code + 1) << (16 - ln)] = (ln << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


def _extend(v, s):
    return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1


def coefficients(p):
    """-> int64 [MCU rows * MCU cols * blocks per MCU, 64]: quantised coefficients in natural order, the DC already summed up, in the order
    of the scan (per MCU: the luma blocks row by row, Cb, Cr).  Sequential: restart interval after restart interval, MCU after MCU."""
    my, mx = p.mcus
    nl = p.hs * p.vs
    bpm = p.blocks_per_mcu
    dc = {k: _lut(*v) for k, v in p.dc.items()}
    ac = {k: _lut(*v) for k, v in p.ac.items()}
    zz = [int(v) for v in jpeg.ZIGZAG]
    out = np.zeros((my * mx * bpm, 64), np.int64)
    markers = re.findall(b'\xff[\xd0-\xd7]', p.scan)
    intervals = re.split(b'\xff[\xd0-\xd7]', p.scan)
    nmcu = my * mx
    per = p.restart if p.restart else nmcu
    assert len(intervals) == (nmcu + per - 1) // per and all(m[1] == 0xD0 + (i & 7) for i, m in enumerate(markers))
    for iv, raw in enumerate(intervals):
        d = raw.replace(b'\xff\x00', b'\xff') + bytes(8)                      # (bits beyond the data read as zeros)
        pos = 0

        def take(lut):
            nonlocal pos
            i = pos >> 3
            e = lut[(((d[i] << 16) | (d[i + 1] << 8) | d[i + 2]) >> (8 - (pos & 7))) & 0xFFFF]
            assert e, 'undefined Huffman code'
            pos += e >> 8
            return e & 255

        def value(s):
            nonlocal pos
            if s == 0:
                return 0
            i = pos >> 3
            v = ((((d[i] << 16) | (d[i + 1] << 8) | d[i + 2]) >> (8 - (pos & 7))) & 0xFFFF) >> (16 - s)
            pos += s
            return _extend(v, s)

        pred = [0, 0, 0]
        for m in range(iv * per, min((iv + 1) * per, nmcu)):
            for b in range(bpm):
                c = 0 if b < nl else b - nl + 1
                blk = out[m * bpm + b]
                s = take(dc[p.td[c]])
                assert s <= 11
                pred[c] += value(s)
                blk[0] = pred[c]
                k = 1
                lut = ac[p.ta[c]]
                while k < 64:
                    rs = take(lut)
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    assert k < 64
                    blk[zz[k]] = value(s)
                    k += 1
        assert (pos + 7) >> 3 == len(d) - 8, (iv, pos, len(d) - 8)             # the interval ends inside its last byte
    return out


def idct_blocks(q, qtab):
    """q [B, 64] quantised, natural order; qtab [64] -> samples [B, 8, 8] in 0 .. 255."""
    c = np.clip(q * np.asarray(qtab, np.int64)[None, :], -32767, 32767).reshape(-1, 8, 8)       # [B, v, u]
    s1 = np.einsum('vy,bvu->byu', T, c)
    assert np.abs(s1).max(initial=0) < 2 ** 30
    t = np.clip((s1 + 512) >> 10, -65535, 65535)
    s2 = np.einsum('ux,byu->byx', T, t)
    assert np.abs(s2).max(initial=0) < 2 ** 31 - 32768
    return np.clip(((s2 + 32768) >> 16) + 128, 0, 255)


def planes(p, coef=None):
    """-> the component planes at MCU-padded size: [Y] or [Y, Cb, Cr], int64."""
    coef = coefficients(p) if coef is None else coef
    my, mx = p.mcus
    bpm, nl = p.blocks_per_mcu, p.hs * p.vs
    c = coef.reshape(my, mx, bpm, 64)
    y = idct_blocks(c[:, :, :nl].reshape(-1, 64), p.qtabs[p.tq[0]]).reshape(my, mx, p.vs, p.hs, 8, 8)
    out = [y.transpose(0, 2, 4, 1, 3, 5).reshape(my * p.vs * 8, mx * p.hs * 8)]
    for k in range(1, p.ncomp):
        s = idct_blocks(c[:, :, nl + k - 1].reshape(-1, 64), p.qtabs[p.tq[k]]).reshape(my, mx, 8, 8)
        out.append(s.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
    return out


def upsample(c, p):
    """A chroma plane (MCU-padded) -> [h, w] by the triangle filter; neighbours clamped to the component's real size."""
    h, w = p.h, p.w
    if p.hs == 1:
        return c[:h, :w]
    cw = (w + 1) // 2
    x = np.arange(w)
    cx = x >> 1
    other = np.clip(np.where(x & 1, cx + 1, cx - 1), 0, cw - 1)
    if p.vs == 1:
        a, b = c[:h][:, cx], c[:h][:, other]
        return (3 * a + b + np.where(x & 1, 2, 1)[None, :]) >> 2
    ch = (h + 1) // 2
    y = np.arange(h)
    cy = y >> 1
    far = np.clip(np.where(y & 1, cy + 1, cy - 1), 0, ch - 1)
    v = 3 * c[cy] + c[far]                                                          # [h, padded width]
    return (3 * v[:, cx] + v[:, other] + np.where(x & 1, 7, 8)[None, :]) >> 4


def pixels(p, coef=None):
    """-> uint8 [h, w, 3]"""
    pl = planes(p, coef)
    y = pl[0][:p.h, :p.w]
    if p.ncomp == 1:
        return np.repeat(y[..., None], 3, axis=2).astype(np.uint8)
    cb, cr = upsample(pl[1], p) - 128, upsample(pl[2], p) - 128
    k = jpeg.COLOUR
    r = y + ((k[0] * cr + 32768) >> 16)
    g = y + ((-k[1] * cb - k[2] * cr + 32768) >> 16)
    b = y + ((k[3] * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


_cache = {}


def decode(data):
    """A file's bytes -> uint8 [h, w, 3] by the rule; computed once per session and file, the result is read-only."""
    data = bytes(data)
    if data not in _cache:
        out = pixels(jpeg.parse_baseline(data))
        out.setflags(write=False)
        _cache[data] = out
    return _cache[data]


# ---- the pictures and files the CPU and the GPU tests share --------------------------------------------------------------------------
def smooth(h, w, seed=0):
    """Low-frequency colour gradients with a little texture: what a camera picture looks like to a JPEG coder."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = 2.0 * np.pi / max(h, w, 8)
    ch = [127.5 + 100.0 * np.sin(f * (xx * (1 + k) + yy * (2 - k)) + seed + k) + 20.0 * np.cos(f * 5.0 * (xx - yy * k)) for k in range(3)]
    return np.clip(np.rint(np.stack(ch, axis=2)), 0, 255).astype(np.uint8)


def noise(h, w, seed=7):
    return np.random.default_rng(seed + 1000 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def pil_file(img, mode='RGB', **kw):
    """The JPEG PIL writes for a picture (kw: quality, subsampling, optimize, restart_marker_blocks, restart_marker_rows, progressive)."""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).convert(mode).save(b, 'JPEG', **kw)
    return b.getvalue()


def pil_pixels(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    return np.asarray(im.convert('RGB'))


SIZES = [(1, 1), (8, 8), (9, 9), (16, 16), (17, 33), (7, 640), (640, 7), (96, 128), (224, 320)]
LAYOUTS = (('RGB', 0), ('RGB', 1), ('RGB', 2), ('L', None))                 # PIL's subsampling 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0, and grey


def layout_kw(layout):
    mode, sub = layout
    return dict(mode=mode) if sub is None else dict(mode=mode, subsampling=sub)


def size_picture(h, w):
    return smooth(h, w) if (h, w) == (224, 320) else noise(h, w)


def batch_files(n=33):
    """n files cycling through SIZES, the four layouts and three qualities (the first: 96 x 128 noise, 4:2:0, quality 100)."""
    out = []
    for i in range(n):
        h, w = SIZES[(7 + i) % len(SIZES)]
        q = (100, 75, 1)[i % 3] if i else 100
        out.append(pil_file(size_picture(h, w), quality=q, **layout_kw(LAYOUTS[(2 + i) % 4])))
    return out
