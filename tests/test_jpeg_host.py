"""The host side of the GPU JPEG encoder (jpeg.py) and the numpy restatement of its rule (tests/jpeg_ref.py) against PIL, the independent
implementation: tables, decodability, fidelity and size beside PIL's own encoder, the literal bytes of a hand-built case, and the input
conditions the GPU test (test_gpu_jpeg.py) relies on - so that it cannot hide a path its pictures never entered.  DESIGN.md 3.12."""
import io
import sys
from pathlib import Path

import numpy as np
import pytest
from PIL import Image, ImageFile, JpegImagePlugin

from k210_yolo_framework_amd import jpeg
from tests import jpeg_ref

ROOT = Path(__file__).resolve().parent.parent


def _pil_bytes(arr, q):
    b = io.BytesIO()
    Image.fromarray(arr).save(b, 'JPEG', quality=q, subsampling=2, optimize=False)
    return b.getvalue()


def _psnr(a, b):
    return 10.0 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


@pytest.mark.parametrize('q', [1, 10, 49, 50, 75, 95, 100])
def test_quant_tables_are_pils(q):
    im = Image.open(io.BytesIO(_pil_bytes(np.zeros((16, 16, 3), np.uint8), q)))
    ours = jpeg.quant_tables(q)
    for i in range(2):
        theirs = np.asarray(im.quantization[i])
        # Pillow has reported the tables in natural order since 8.3 and in zigzag order before
        assert np.array_equal(theirs, ours[i]) or np.array_equal(theirs, ours[i][jpeg.ZIGZAG]), (q, i)
    assert ours.dtype == np.uint8 and ours.min() >= 1
    with pytest.raises(ValueError):
        jpeg.quant_tables(0)
    with pytest.raises(ValueError):
        jpeg.quant_tables(101)


def test_tables_are_annex_k():
    for bits, vals in ((jpeg.DC_LUMA_BITS, jpeg.DC_LUMA_VALS), (jpeg.DC_CHROMA_BITS, jpeg.DC_CHROMA_VALS),
                       (jpeg.AC_LUMA_BITS, jpeg.AC_LUMA_VALS), (jpeg.AC_CHROMA_BITS, jpeg.AC_CHROMA_VALS)):
        assert len(bits) == 16 and sum(bits) == len(vals) == len(set(vals))
        code, length = jpeg.huffman_codes(bits, vals)
        words = sorted(format(int(code[s]), f'0{int(length[s])}b') for s in vals)
        assert all(not b.startswith(a) for a, b in zip(words, words[1:]))             # prefix-free
        assert all(set(w) != {'1'} for w in words)                                    # no code of all ones (T.81 C.2)
    assert sorted(jpeg.ZIGZAG) == list(range(64)) and list(jpeg.ZIGZAG[:6]) == [0, 1, 8, 16, 9, 2]
    # what PIL writes into its own files are the same four tables: its DHT segments, byte for byte
    data = _pil_bytes(np.zeros((8, 8, 3), np.uint8), 75)
    ours = jpeg.headers(8, 8, jpeg.quant_tables(75))
    for tc_th, bits, vals in jpeg.HUFFMAN_TABLES:
        body = bytes([tc_th]) + bytes(bits) + bytes(vals)
        assert body in data and body in ours


def test_device_tables_header_is_generated_from_jpeg_py():
    sys.path.insert(0, str(ROOT / 'tools'))
    try:
        import gen_jpeg_tables
    finally:
        sys.path.pop(0)
    assert (ROOT / 'k210_yolo_framework_amd' / 'csrc' / 'yk_jpeg_tables.h').read_text() == gen_jpeg_tables.render()


def test_clamps_are_out_of_reach_of_8_bit_pixels():
    """The +-1023 / +-2047 clamps of the rule are safety nets.  Interval arithmetic through the two passes with s in [-128, 127] and d = 1:
    no AC coefficient exceeds 1020 and the DC lies in [-1024, 1016], so no DC difference exceeds 2040: no picture can
    exercise the clamps - hence none of the test set does - and the intermediate bounds of the rule hold."""
    T = jpeg_ref.T
    pos, neg = np.where(T > 0, T, 0).sum(axis=1), np.where(T < 0, -T, 0).sum(axis=1)
    r_hi, r_lo = pos * 127 + neg * 128, -(pos * 128 + neg * 127)
    assert max(r_hi.max(), -r_lo.min()) < 2 ** 22
    r1_hi, r1_lo = (r_hi + 512) >> 10, (r_lo + 512) >> 10
    assert max(r1_hi.max(), -r1_lo.min()) <= 4018
    c_hi = pos[:, None] * r1_hi[None, :] + neg[:, None] * -r1_lo[None, :]
    c_lo = -(pos[:, None] * -r1_lo[None, :] + neg[:, None] * r1_hi[None, :])
    assert max(c_hi.max(), -c_lo.min()) < 1.3e8 and -c_lo.min() + 255 * 32768 < 2 ** 31
    q_hi, q_lo = (c_hi + 32768) >> 16, -((-c_lo + 32768) >> 16)
    assert q_hi[0, 0] == 1016 and q_lo[0, 0] == -1024
    assert max(np.delete(q_hi.reshape(-1), 0).max(), -np.delete(q_lo.reshape(-1), 0).min()) == 1020
    # the extremes are reached: a black and a white block, and the 0 / 255 pattern of basis function (0, 4)
    ones = np.ones(64, np.int64)
    black, white = (jpeg_ref.block_coefficients(np.full((8, 8), v, np.int64), ones)[0][0, 0, 0] for v in (0, 255))
    assert (int(black), int(white)) == (-1024, 1016)
    stripes = np.where(T[4] > 0, 255, 0)[None, :].repeat(8, axis=0)
    assert int(jpeg_ref.block_coefficients(stripes, ones)[0][0, 0, 4]) == 1020


@pytest.mark.parametrize('q', jpeg_ref.QUALITIES)
def test_every_file_decodes(q):
    assert ImageFile.LOAD_TRUNCATED_IMAGES is False
    for i, pic in enumerate(jpeg_ref.batch_pictures()):
        scan, _ = jpeg_ref.encode_cached(i, q)
        data = jpeg.assemble(pic.shape[0], pic.shape[1], jpeg.quant_tables(q), scan)
        im = Image.open(io.BytesIO(data))
        assert im.format == 'JPEG' and im.mode == 'RGB' and im.size == (pic.shape[1], pic.shape[0]), i
        assert JpegImagePlugin.get_sampling(im) == 2
        im.load()
        # no trailing and no missing bytes: libjpeg stops reading at EOI, and a file cut by one byte no longer loads
        assert data.endswith(b'\xff\xd9') and data.count(b'\xff\xd9') >= 1
        if pic.shape == (96, 128, 3):
            cut = Image.open(io.BytesIO(data[:-3]))
            with pytest.raises(OSError):
                cut.load()


def _sources():
    smooth = np.asarray(Image.open(ROOT / 'data' / 'synthetic_320x224.jpg').convert('RGB'))
    return {'smooth': smooth, 'noise': jpeg_ref.picture('noise', 96, 128)}


# measured here with jpeg_ref against Pillow 12.2 / its libjpeg: PSNR deficit in dB and size excess in % of PIL's file
#   smooth  q50 +0.015 dB -1.00 %   q75 +0.053 dB -0.04 %   q95 +0.032 dB -0.04 %
#   noise   q50 +0.001 dB -0.16 %   q75 -0.002 dB +0.01 %   q95 -0.000 dB -0.02 %
# bars: the largest measured gap (+0.053 dB, +0.01 %) rounded up to the next 0.1 dB / the next 1 %.
PSNR_BAR_DB = 0.1
SIZE_BAR_PERCENT = 1.0


@pytest.mark.parametrize('name', ['smooth', 'noise'])
@pytest.mark.parametrize('q', [50, 75, 95])
def test_fidelity_and_size_beside_pil(name, q):
    src = _sources()[name]
    ours = jpeg_ref.file(src, q)
    theirs = _pil_bytes(src, q)
    a, b = Image.open(io.BytesIO(ours)), Image.open(io.BytesIO(theirs))
    assert a.quantization == b.quantization and JpegImagePlugin.get_sampling(a) == JpegImagePlugin.get_sampling(b) == 2
    deficit = _psnr(np.asarray(b), src) - _psnr(np.asarray(a), src)
    excess = 100.0 * (len(ours) / len(theirs) - 1.0)
    print(f'{name} q{q}: PSNR deficit {deficit:+.3f} dB, size excess {excess:+.2f} %')
    assert deficit <= PSNR_BAR_DB
    assert excess <= SIZE_BAR_PERCENT


def test_flat_grey_8x8_literal_bytes():
    """An 8 x 8 picture of (128, 128, 128): Y = Cb = Cr = 128, every sample 0, so each of the six blocks of its one MCU is the DC code of
    category 0 and EOB - luminance '00' + '1010' four times, chrominance '00' + '00' twice: 32 bits, which end on a byte boundary, so nothing is padded."""
    pic = np.full((8, 8, 3), 128, np.uint8)
    scan, st = jpeg_ref.encode(pic, 75)
    assert st['bits'] == 32 and st['eob_only'] == 6 and st['blocks'] == 6
    want_scan = int('001010' * 4 + '0000' * 2, 2).to_bytes(4, 'big')
    assert scan == want_scan == bytes([0x28, 0xA2, 0x8A, 0x00])
    qt = jpeg.quant_tables(75)
    data = jpeg.assemble(8, 8, qt, scan)
    want = bytes.fromhex('ffd8' 'ffe000104a46494600010100000100010000')
    want += bytes.fromhex('ffdb004300') + bytes(int(v) for v in qt[0][jpeg.ZIGZAG])
    want += bytes.fromhex('ffdb004301') + bytes(int(v) for v in qt[1][jpeg.ZIGZAG])
    want += bytes.fromhex('ffc0001108' '0008' '0008' '03' '012200' '021101' '031101')
    want += bytes.fromhex('ffc4001f00') + bytes(jpeg.DC_LUMA_BITS) + bytes(jpeg.DC_LUMA_VALS)
    want += bytes.fromhex('ffc400b510') + bytes(jpeg.AC_LUMA_BITS) + bytes(jpeg.AC_LUMA_VALS)
    want += bytes.fromhex('ffc4001f01') + bytes(jpeg.DC_CHROMA_BITS) + bytes(jpeg.DC_CHROMA_VALS)
    want += bytes.fromhex('ffc400b511') + bytes(jpeg.AC_CHROMA_BITS) + bytes(jpeg.AC_CHROMA_VALS)
    want += bytes.fromhex('ffda000c03' '0100' '0211' '0311' '003f00') + want_scan + bytes.fromhex('ffd9')
    assert data == want
    assert list(qt[0][:4]) == [8, 6, 5, 8] and list(qt[1][:4]) == [9, 9, 12, 24]      # quality 75: scale 50
    im = Image.open(io.BytesIO(data))
    assert np.abs(np.asarray(im).astype(int) - 128).max() <= 1
    with pytest.raises(ValueError):
        jpeg.headers(0, 8, qt)
    with pytest.raises(ValueError):
        jpeg.headers(8, 65536, qt)


def test_input_conditions_of_the_gpu_test():
    tot = dict(stuffed=0, zrl=0, eob_only=0, clamped_ac=0, clamped_dc=0)
    aligned = ragged = 0
    big_dc = 0
    for q in jpeg_ref.QUALITIES:
        for i, pic in enumerate(jpeg_ref.batch_pictures()):
            scan, st = jpeg_ref.encode_cached(i, q)
            for k in tot:
                tot[k] += st[k]
            aligned += st['bits'] % 8 == 0
            ragged += st['bits'] % 8 != 0
            assert len(scan) == (st['bits'] + 7) // 8 + st['stuffed']
    assert tot['stuffed'] > 0 and tot['zrl'] > 0 and tot['eob_only'] > 0
    assert aligned > 0 and ragged > 0                      # streams that end on a byte boundary, and streams that are padded
    assert tot['clamped_ac'] == 0 and tot['clamped_dc'] == 0       # out of reach: test_clamps_are_out_of_reach_of_8_bit_pixels
    # the noise picture at quality 95 gives stuffed bytes too (the fidelity test's source)
    assert jpeg_ref.encode(jpeg_ref.picture('noise', 96, 128), 95)[1]['stuffed'] > 0
    # the black / white cells at quality 100 reach the longest DC category
    for i, pic in enumerate(jpeg_ref.batch_pictures()):
        if i % len(jpeg_ref.KINDS) == 4 and min(pic.shape[:2]) > 16:
            y = jpeg_ref.planes(pic)[0]
            dc = jpeg_ref.block_coefficients(y, jpeg.quant_tables(100)[0])[0][..., 0]
            big_dc += int(np.abs(np.diff(dc, axis=1)).max(initial=0) >= 1024)
    assert big_dc > 0
