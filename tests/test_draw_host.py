"""Host side of `make detect` (no GPU): the label rule against Python's formatting, the ragged packing and its table, the glyph table,
and detect.py's argument parsing, folder expansion, extension filter and output names."""
import numpy as np
import pytest

from k210_yolo_framework_amd import detect, draw

TIES = [0.0, 0.005, 0.125, 0.285, 0.995, 1.0]


def _want(cls, score):
    return [draw.GLYPHS.index(ch) for ch in '{:2d} {:.2f}'.format(int(cls), float(np.float32(score)))]


def test_label_glyphs_equal_python_formatting_over_fp32_scores():
    rng = np.random.default_rng(11)
    scores = np.concatenate([rng.random(10000, dtype=np.float32), np.asarray(TIES, np.float32),
                             np.arange(0, 201, dtype=np.float32) / np.float32(200)])                   # every x.xx5 the format can tie on
    classes = rng.integers(0, 100, len(scores))
    for c, s in zip(classes, scores):
        assert draw.label_glyphs(c, s) == _want(c, s), (c, float(s))
    for c in (0, 7, 19):
        for s in TIES:
            g = draw.label_glyphs(c, s)
            assert len(g) == draw.LABEL_LEN and g == _want(c, s)
    assert draw.label_glyphs(7, 0.125) == _want(7, 0.125) == [11, 7, 11, 0, 10, 1, 2]                    # the tie goes to even, as Python's
    # outside the label's range the rule is still defined: low digits
    assert draw.label_glyphs(105, 12.344) == [0, 5, 11, 2, 10, 3, 4]
    assert draw.label_glyphs(-3, float('nan')) == [11, 0, 11, 0, 10, 0, 0]


def test_pack_ragged_table_offsets_shapes_and_total():
    rng = np.random.default_rng(3)
    shapes = [(1, 1), (1, 37), (37, 1), (30, 40), (97, 131)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    packed, table, got_shapes = draw.pack_ragged(imgs)
    assert got_shapes == shapes and table.dtype == draw.RAGGED_DTYPE and table.dtype.itemsize == 40
    assert packed.numel() == sum(3 * h * w for h, w in shapes) == draw.packed_bytes(table)
    off = 0
    flat = packed.numpy()
    for row, im in zip(table, imgs):
        assert int(row['offset']) == off and (int(row['h']), int(row['w'])) == im.shape[:2]
        assert np.array_equal(flat[off:off + im.size].reshape(im.shape), im)
        assert int(row['thickness']) == max(1, (im.shape[0] + im.shape[1]) // 300) and int(row['mag']) == 1
        off += im.size
    assert any(int(o) % 2 for o in table['offset'])                                                    # 3-byte pixels: odd offsets happen
    for view, im in zip(draw.unpack_ragged(flat, table), imgs):
        assert np.array_equal(view, im)
    # gaps, and the per-picture rules
    _, gapped, _ = draw.pack_ragged(imgs, gap=5)
    assert [int(o) for o in gapped['offset']] == [int(o) + 5 * i for i, o in enumerate(table['offset'])]
    assert draw.thickness_of(240, 320) == 1 and draw.thickness_of(375, 500) == 2 and draw.thickness_of(1100, 64) == 3
    assert draw.magnification_of(240) == 1 and draw.magnification_of(1049) == 1 and draw.magnification_of(1100) == 2
    with pytest.raises(ValueError):
        draw.pack_ragged([np.zeros((0, 4, 3), np.uint8)])
    with pytest.raises(ValueError):
        draw.pack_ragged([np.zeros((4, 4), np.uint8)])


def test_glyph_table_is_binary_distinct_and_the_space_is_empty():
    atlas = draw.glyph_atlas()
    assert atlas.shape == (12, 16, 8) and atlas.dtype == np.uint8 and len(draw.GLYPHS) == 12
    assert set(np.unique(atlas).tolist()) == {0, 1}
    assert not atlas[draw.GLYPHS.index(' ')].any()
    for i in range(12):
        for j in range(i + 1, 12):
            assert not np.array_equal(atlas[i], atlas[j]), (draw.GLYPHS[i], draw.GLYPHS[j])
    assert not atlas[:, :, 0].any() and not atlas[:, :, 7].any()                                         # neighbouring cells never touch
    assert all(atlas[i].any() for i in range(11))


def test_detect_arguments_sources_and_output_names(tmp_path):
    a = detect.parse(['w.h5', 'pics', '--out_dir', 'o', '--draw', 'False', '--batch', '4', '--depth', '2', '--precision', 'f16',
                      '--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.75', '--obj_thresh', '0.3'])
    assert (a.pre_ckpt, a.src, a.out_dir, a.draw, a.batch, a.depth, a.precision) == ('w.h5', 'pics', 'o', False, 4, 2, 'f16')
    assert a.model_def == 'yolo_mobilev1' and a.depth_multiplier == 0.75 and a.obj_thresh == 0.3 and a.iou_thresh == 0.3
    d = detect.parse(['w.h5', 'pics'])
    assert d.draw is True and d.out_dir == 'out' and d.batch == 32 and d.depth == 4 and d.precision == 'f16x2'
    for bad in (['w.h5', 'pics', '--precision', 'kpu'], ['w.kmodel', 'pics'], ['w.h5', 'pics', '--batch', '0'], ['w.h5', 'pics', '--draw', 'yes']):
        with pytest.raises(SystemExit):
            detect.parse(bad)
    assert detect.MAX_WORKERS == 16

    folder = tmp_path / 'pics'
    folder.mkdir()
    for name in ('b.jpg', 'a.PNG', 'c.jpeg', 'd.bmp', 'notes.txt', 'e.gif', 'f.jpg.bak'):
        (folder / name).write_bytes(b'x')
    (folder / 'sub.jpg').mkdir()                                                                        # a folder is not a picture
    got = detect.expand_sources(folder)
    assert got == [str(folder / n) for n in ('a.PNG', 'b.jpg', 'c.jpeg', 'd.bmp')]
    assert detect.expand_sources(folder / 'b.jpg') == [str(folder / 'b.jpg')]
    lst = tmp_path / 'list.txt'
    lst.write_text(f'# pictures\n{folder / "b.jpg"}\n\npics/a.PNG\n')
    assert detect.expand_sources(lst) == [str(folder / 'b.jpg'), str(tmp_path / 'pics' / 'a.PNG')]
    with pytest.raises(FileNotFoundError):
        detect.expand_sources(tmp_path / 'nothing')
    names = detect.output_names(['x/dog.jpg', 'y/cat.png', 'z/dog.bmp'], 'out')
    assert names == ['out/dog_res.jpg', 'out/cat_res.jpg', 'out/dog_2_res.jpg']
