"""engine.check_{ragged,tile,view}_rows - one implementation behind three row types - on host rows each kind must refuse, against the exact
YkError text (no GPU, no library: numpy only).  The expected strings are literals, recorded from the three separate functions these replaced."""
import numpy as np
import pytest

from k210_yolo_framework_amd import draw, engine, tiles, tta

M = 2 ** 31 - 1
KINDS = {'ragged': (engine.check_ragged_rows, draw.RAGGED_DTYPE, {}),
         'tile': (engine.check_tile_rows, tiles.TILE_DTYPE, dict(stride=15)),
         'view': (engine.check_view_rows, tta.VIEW_DTYPE, dict(ch=8, cw=8))}

# (kind, the fields of one row that is otherwise a 4 x 5 picture at offset 0, packed_bytes, the message or None for a row that passes)
ROWS = [
    ('ragged', dict(h=0), 100, 'ragged table: row 1 is 0 x 5'),
    ('ragged', dict(w=-1), 100, 'ragged table: row 1 is 4 x -1'),
    ('ragged', dict(offset=41), 100, 'ragged table: row 1 ends at byte 101 of a 100-byte buffer'),
    ('ragged', dict(offset=40), 100, None),
    ('tile', dict(h=0), 100, 'tile table: row 1 is 0 x 5'),
    ('tile', dict(w=-1), 100, 'tile table: row 1 is 4 x -1'),
    ('tile', dict(stride=14), 100, 'tile table: row 1 has stride 14, less than the 15 bytes of one of its rows'),
    ('tile', dict(offset=26, stride=20), 100, 'tile table: row 1 ends at byte 101 of a 100-byte buffer'),       # 26 + 3 * 20 + 15
    ('tile', dict(offset=25, stride=20), 100, None),
    ('view', dict(h=0), 100, 'view table: row 1 is 0 x 5'),
    ('view', dict(w=-1), 100, 'view table: row 1 is 4 x -1'),
    ('view', dict(oy=5), 100, 'view table: row 1 puts its 4 x 5 picture at (5, 0), outside its canvas of 8 x 8'),           # oy + h = ch + 1
    ('view', dict(oy=4), 100, None),
    ('view', dict(ox=-1), 100, 'view table: row 1 puts its 4 x 5 picture at (0, -1), outside its canvas of 8 x 8'),
    # oy + h = 2^32 - 2 is -2 in 32 bits, which would lie inside the canvas
    ('view', dict(h=M, w=M, ch=M, cw=M, oy=M), 100,
     'view table: row 1 puts its 2147483647 x 2147483647 picture at (2147483647, 0), outside its canvas of 2147483647 x 2147483647'),
    ('view', dict(offset=41), 100, 'view table: row 1 ends at byte 101 of a 100-byte buffer'),
    ('view', dict(offset=40), 100, None),
]


@pytest.mark.parametrize('kind,fields,packed_bytes,message', ROWS, ids=[f'{r[0]}-{"-".join(f"{k}{v}" for k, v in r[1].items())}' for r in ROWS])
def test_a_bad_row_is_refused_in_these_words(kind, fields, packed_bytes, message):
    check, dtype, base = KINDS[kind]
    t = np.zeros(2, dtype)                       # row 0 is good: the message names the row
    for name, v in dict(h=4, w=5, **base).items():
        t[name] = v
    for name, v in fields.items():
        t[name][1] = v
    before = t.copy()
    if message is None:
        got = check(t, packed_bytes)
        assert got.dtype == dtype and got.shape == (2,) and got is not t and np.array_equal(got, before)
    else:
        with pytest.raises(engine.YkError) as e:
            check(t, packed_bytes)
        assert str(e.value) == message
    assert np.array_equal(t, before)


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_an_empty_table_passes_the_check(kind):
    check, dtype, _ = KINDS[kind]
    got = check(np.zeros(0, dtype), 0)
    assert got.dtype == dtype and got.shape == (0,)
