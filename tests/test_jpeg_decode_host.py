"""Host side of the GPU JPEG decoder: jpeg.parse_baseline on every layout PIL writes and on what it must refuse by name,
jpeg.plan_decode's layout, the generated table header, the interval arithmetic of the IDCT, and the rule itself - tests/jpeg_dec_ref.py -
against PIL's decoder on a fixed fixture set: a worst case derived from the arithmetic, a mean measured once and recorded."""
import io
import sys
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import jpeg
from tests import jpeg_dec_ref as ref, jpeg_ref

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden'


def _pil_cases():
    pic = ref.noise(33, 47)
    out = []
    for lay in ref.LAYOUTS:
        for opt in (False, True):
            out.append((f'{lay} optimize={opt}', ref.pil_file(pic, optimize=opt, **ref.layout_kw(lay)), lay, 0))
    for q in (1, 75, 100):
        out.append((f'quality {q}', ref.pil_file(pic, quality=q), ('RGB', 2), 0))
    out.append(('restart 1 block', ref.pil_file(pic, restart_marker_blocks=1), ('RGB', 2), 1))
    out.append(('restart 7 blocks', ref.pil_file(pic, restart_marker_blocks=7), ('RGB', 2), 7))
    out.append(('restart 1 row', ref.pil_file(pic, restart_marker_rows=1), ('RGB', 2), 3))           # 47 pixels = 3 MCUs of 16
    return out


def test_parser_accepts_every_layout_pil_writes():
    sampling = {0: (1, 1), 1: (2, 1), 2: (2, 2), None: (1, 1)}
    for name, data, (mode, sub), restart in _pil_cases():
        p = jpeg.parse_baseline(data)
        assert (p.h, p.w) == (33, 47) and p.ncomp == (1 if mode == 'L' else 3), name
        assert (p.hs, p.vs) == sampling[sub] and p.restart == restart, name
        assert len(p.tq) == len(p.td) == len(p.ta) == p.ncomp
        assert all(t in p.qtabs for t in p.tq) and all(t in p.dc for t in p.td) and all(t in p.ac for t in p.ta)
        at = data.index(p.scan)
        assert data[at + len(p.scan):] == b'\xff\xd9' and data[at - 2 - 2 * p.ncomp - 4 - 2:at - 2 - 2 * p.ncomp - 4] == b'\xff\xda', name
        assert (restart > 0) == (b'\xff\xd0' in p.scan), name               # DRI + RSTn are what PIL writes for the restart options
        from PIL import Image
        q = Image.open(io.BytesIO(data)).quantization
        for k, t in p.qtabs.items():
            assert np.array_equal(t, np.asarray(q[k])) or np.array_equal(t[jpeg.ZIGZAG], np.asarray(q[k])), name
    img = jpeg_ref.picture('noise', 17, 9)
    p = jpeg.parse_baseline(jpeg_ref.file(img, 75))                           # the project's own encoder's container
    assert (p.h, p.w, p.ncomp, p.hs, p.vs, p.restart) == (17, 9, 3, 2, 2, 0) and p.scan == jpeg_ref.encode(img, 75)[0]
    assert np.array_equal(np.stack([p.qtabs[0], p.qtabs[1]]), jpeg.quant_tables(75))
    assert p.dc[0] == (bytes(jpeg.DC_LUMA_BITS), bytes(jpeg.DC_LUMA_VALS)) and p.ac[1] == (bytes(jpeg.AC_CHROMA_BITS), bytes(jpeg.AC_CHROMA_VALS))


def _reason(data):
    with pytest.raises(jpeg.Unsupported) as e:
        jpeg.parse_baseline(data)
    assert e.value.reason == str(e.value)
    return e.value.reason


def test_every_refusal_carries_its_reason():
    from PIL import Image
    pic = ref.noise(33, 47)
    good = ref.pil_file(pic)
    assert 'progressive' in _reason(ref.pil_file(pic, progressive=True))
    assert 'four components' in _reason(ref.pil_file(pic, mode='CMYK'))
    b = io.BytesIO()
    Image.fromarray(pic).save(b, 'PNG')
    assert 'not a JPEG' in _reason(b.getvalue())
    assert 'not a JPEG' in _reason(b'')
    assert 'no EOI' in _reason(good[:-2])
    assert 'no EOI' in _reason(good[:len(good) - 200])
    sos = good.index(b'\xff\xda')
    assert 'no SOS' in _reason(good[:sos])
    # edited headers: one byte each
    sof = good.index(b'\xff\xc0')
    edit = lambda at, v: good[:at] + bytes([v]) + good[at + 1:]
    assert '12-bit' in _reason(edit(sof + 4, 12))
    assert 'dimension of 0' in _reason(good[:sof + 5] + b'\x00\x00' + good[sof + 7:])
    assert 'sampling' in _reason(edit(sof + 11, 0x41))                        # luma 4 x 1
    assert 'arithmetic' in _reason(edit(sof + 1, 0xC9))
    assert 'SOF1' in _reason(edit(sof + 1, 0xC1))
    dqt = good.index(b'\xff\xdb')
    assert '16-bit quantisation' in _reason(edit(dqt + 4, 0x10))
    assert 'not Ss 0' in _reason(edit(sos + 2 + 2 + 1 + 6 + 1, 62))
    dht = good.index(b'\xff\xc4')
    assert good[dht + 4] == 0x00 and good[dht + 7] >= 3
    over = good[:dht + 5] + b'\x03' + good[dht + 6:dht + 7] + bytes([good[dht + 7] - 3]) + good[dht + 8:]
    assert 'over-subscribe' in _reason(over)                                  # three codes of one bit, as many values as before
    assert 'DNL' in _reason(good[:sos] + b'\xff\xdc\x00\x04\x00\x21' + good[sos:])
    assert 'more than one scan' in _reason(good[:-2] + good[sos:])
    adobe = b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00'
    assert 'Adobe' in _reason(good[:2] + adobe + b'\x00' + good[2:])          # transform 0: the components are RGB
    assert jpeg.parse_baseline(good[:2] + adobe + b'\x01' + good[2:]).ncomp == 3
    # what is skipped stays accepted: a comment, an APP1, DHT segments merged into one and split into four
    assert jpeg.parse_baseline(good[:2] + b'\xff\xfe\x00\x05abc' + b'\xff\xe1\x00\x04xy' + good[2:]).scan == jpeg.parse_baseline(good).scan
    p = jpeg.parse_baseline(good)
    body = b''.join(bytes([cls << 4 | k]) + bits + vals for cls, tabs in ((0, p.dc), (1, p.ac)) for k, (bits, vals) in tabs.items())
    first, last = good.index(b'\xff\xc4'), good.index(b'\xff\xda')
    merged = good[:first] + b'\xff\xc4' + (len(body) + 2).to_bytes(2, 'big') + body + good[last:]
    q = jpeg.parse_baseline(merged)
    assert q.dc == p.dc and q.ac == p.ac and q.scan == p.scan


def test_plan_layout():
    files = [ref.pil_file(ref.noise(17, 33), quality=75), ref.pil_file(ref.noise(16, 16), mode='L', restart_marker_blocks=1),
             ref.pil_file(ref.smooth(50, 70), subsampling=1, optimize=True)]
    parsed = [jpeg.parse_baseline(f) for f in files]
    buf, pics, scan_bytes, table_bytes = jpeg.plan_decode(parsed)
    assert pics.dtype == jpeg.PIC_DTYPE and jpeg.PIC_DTYPE.itemsize == 56 and table_bytes == 3 * jpeg.PIC_TABLE_BYTES == 3 * 3840
    assert len(buf) == scan_bytes + table_bytes
    end = 0
    for row, p in zip(pics, parsed):
        o, n = int(row['scan_offset']), int(row['scan_bytes'])
        assert o % 4 == 0 and o >= end and buf[o:o + n].tobytes() == p.scan
        end = o + n + 8
        assert not buf[o + n:end].any() and end <= scan_bytes               # at least 8 zero bytes behind every segment
        assert (row['h'], row['w'], row['ncomp'], row['hs'], row['vs'], row['restart']) == (p.h, p.w, p.ncomp, p.hs, p.vs, p.restart)
        t = buf[scan_bytes + int(row['table_offset']):][:jpeg.PIC_TABLE_BYTES]
        for c in range(p.ncomp):
            assert np.array_equal(t[64 * row['tq'][c]:64 * row['tq'][c] + 64], p.qtabs[p.tq[c]])
    out = np.full(len(buf) + 7, 9, np.uint8)
    again = jpeg.plan_decode(parsed, out=out)
    assert again[0] is out and np.array_equal(out[:len(buf)], buf) and (out[len(buf):] == 9).all()


def test_decode_table_decodes_every_code():
    for bits, vals in ((jpeg.AC_LUMA_BITS, jpeg.AC_LUMA_VALS), (jpeg.DC_CHROMA_BITS, jpeg.DC_CHROMA_VALS)):
        t = jpeg.decode_table(bits, vals)
        assert t.dtype == np.uint8 and len(t) == jpeg.HUFF_TABLE_BYTES
        look, maxcode, delta, v = t[:512].view('<u2'), t[512:576].view('<i4'), t[576:640].view('<i4'), t[640:]
        code, length = jpeg.huffman_codes(bits, vals)
        for sym in vals:
            ln, c = int(length[sym]), int(code[sym])
            if ln <= 8:
                for tail in (0, (1 << (8 - ln)) - 1):
                    assert look[(c << (8 - ln)) | tail] == (ln << 8 | sym)
            else:
                assert look[c >> (ln - 8)] == 0 and c <= maxcode[ln - 1] and v[c + delta[ln - 1]] == sym
                assert all(maxcode[k - 1] < (c >> (ln - k)) for k in range(1, ln))     # no shorter length claims its prefix
        assert look[255] == 0 and all(maxcode[k - 1] < (0xFFFF >> (16 - k)) for k in range(1, 17))  # the all-ones code is undefined


def test_decoder_tables_header_is_generated_from_jpeg_py():
    sys.path.insert(0, str(ROOT / 'tools'))
    try:
        import gen_jpeg_dec_tables
    finally:
        sys.path.pop(0)
    assert (ROOT / 'k210_yolo_framework_amd' / 'csrc' / 'yk_jpeg_dec_tables.h').read_text() == gen_jpeg_dec_tables.render()
    assert np.array_equal(jpeg.idct_table(), jpeg.dct_table())                # the transpose of the encoder's transform: the same matrix


def test_idct_intermediates_fit_int32_for_any_input():
    """Interval arithmetic of the rule (include/yolo_hip.h): with |c| <= 32767 the column sums stay below 2^30, with |t| <= 65535 the row
    sums below 2^31 - 2^15; and coefficients an encoder derives from 8-bit samples (|DCT| <= 1024 per coefficient, half a quantiser step of
    255 on top) leave |t| far inside its clamp."""
    s = int(np.abs(ref.T).sum(axis=0).max())
    assert s == 21641
    assert 32767 * s + 512 < 2 ** 30 and 65535 * s + 32768 < 2 ** 31
    assert ((1024 + 128) * s + 512) >> 10 < 65535 // 2
    worst = np.stack([np.where(ref.T[:, y] >= 0, 32767, -32767)[:, None].repeat(8, 1).reshape(64) for y in range(8)])   # c[v][u] = +-max by T[v][y]
    out = ref.idct_blocks(worst.astype(np.int64), np.ones(64, np.int64))      # runs its own assertions on the sums
    assert out.min() >= 0 and out.max() <= 255
    garbage = np.random.default_rng(1).integers(-32768, 32768, (256, 64))
    ref.idct_blocks(garbage, np.full(64, 255, np.int64))


# ---- the rule against PIL's decoder ---------------------------------------------------------------------------------------------------
# Worst case per channel: two IDCTs that meet IEEE 1180 differ by at most 2 per sample; upsampling with identical weights
# and roundings is monotone and carries at most that through; the colour transform adds ceil(1.402 * 2) = 3 to R, ceil((0.34414 +
# 0.71414) * 2) = 3 to G and ceil(1.772 * 2) = 4 to B, its rounding being the same function of the same integers: 5, 5, 6; grey 2.
MAX_DIFF = 6
# The mean absolute difference measured against Pillow 12.2.0 (libjpeg-turbo) per fixture, recorded in DESIGN.md 3.12; the bar is the
# largest of them plus a quarter - the margin is for a PIL built against another libjpeg, not for the code under test.
MEASURED_MEAN = {'synthetic_320x224': 0.0811, 'dog': 0.0888, 'people': 0.0692, 'smooth 4:4:4': 0.0510, 'smooth 4:2:2': 0.0517,
                 'smooth 4:2:0': 0.0519, 'smooth grey': 0.0255, 'noise 4:4:4': 0.0794, 'noise 4:2:2': 0.0824, 'noise 4:2:0': 0.0826,
                 'noise grey': 0.0360, 'noise q100': 0.0558, 'noise q1': 0.0019}
MEAN_BAR = max(MEASURED_MEAN.values()) + 0.25


def fixtures():
    out = {'synthetic_320x224': (ROOT / 'data' / 'synthetic_320x224.jpg').read_bytes(), 'dog': (GOLDEN / 'jpeg_dog.jpg').read_bytes(),
           'people': (GOLDEN / 'jpeg_people.jpg').read_bytes()}
    for name, lay in zip(('4:4:4', '4:2:2', '4:2:0', 'grey'), ref.LAYOUTS):
        out[f'smooth {name}'] = ref.pil_file(ref.smooth(97, 131), quality=75, **ref.layout_kw(lay))
        out[f'noise {name}'] = ref.pil_file(ref.noise(96, 128), quality=75, **ref.layout_kw(lay))
    out['noise q100'] = ref.pil_file(ref.noise(96, 128), quality=100)
    out['noise q1'] = ref.pil_file(ref.noise(96, 128), quality=1)
    return out


def test_reference_sits_next_to_pils_decoder():
    fx = fixtures()
    assert set(fx) == set(MEASURED_MEAN)
    p = jpeg.parse_baseline(fx['people'])
    assert (p.h, p.w, p.hs, p.vs) == (374, 499, 2, 2)                          # odd sizes: the last MCU column and row are padding
    for name, data in fx.items():
        ours, theirs = ref.decode(data), ref.pil_pixels(data)
        assert ours.shape == theirs.shape and ours.dtype == np.uint8, name
        if 'grey' in name:
            assert np.array_equal(ours[..., 0], ours[..., 1]) and np.array_equal(ours[..., 0], ours[..., 2])
        d = np.abs(ours.astype(np.int64) - theirs.astype(np.int64))
        print(f'{name}: max {int(d.max())} mean {d.mean():.4f}')
        assert d.max() <= (2 if 'grey' in name else MAX_DIFF), (name, int(d.max()))
        assert d[..., 0].max() <= 5 and d[..., 1].max() <= 5, name
        assert d.mean() <= MEAN_BAR, (name, float(d.mean()))


def test_restart_files_decode_like_their_plain_twins():
    """A restart interval changes the stream, not the picture: the coefficients of the same picture with and without DRI are equal."""
    for sub in (0, 2):
        pic = ref.noise(33, 47)
        plain = ref.coefficients(jpeg.parse_baseline(ref.pil_file(pic, subsampling=sub)))
        for kw in (dict(restart_marker_blocks=1), dict(restart_marker_blocks=7), dict(restart_marker_rows=1)):
            assert np.array_equal(ref.coefficients(jpeg.parse_baseline(ref.pil_file(pic, subsampling=sub, **kw))), plain)
