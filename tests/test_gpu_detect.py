"""`make detect` end to end, small: six generated pictures of three sizes through detect.py (batch 4 -> a partial last batch, two batches
in flight), against inference.detect on the same pictures under the project's north-star comparison, and the annotated pictures against the
painter of test_gpu_draw.py applied to the rows of detections.json."""
import json

import numpy as np
import pytest

from k210_yolo_framework_amd import netspec as ns
from k210_yolo_framework_amd.helper import Helper, VOC_ANCHORS
from tests.test_gpu_draw import paint
from tests.test_gpu_e2e import _assert_north_star

pytestmark = pytest.mark.gpu
SIZES = [(240, 320), (375, 500), (333, 250)]
OBJ, IOU = 0.6, 0.5


def _pictures(folder):
    from PIL import Image
    rng = np.random.default_rng(21)
    paths = []
    for i in range(6):
        h, w = SIZES[i % 3]
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)          # seeded noise, the input of the existing end-to-end tests
        p = folder / f'pic{i}.png'                                   # lossless: both paths decode the same pixels
        Image.fromarray(img).save(p)
        paths.append(str(p))
    (folder / 'readme.txt').write_text('not a picture')
    return paths


def test_detect_cli_json_pictures_and_painter(tmp_path, capsys):
    from PIL import Image
    from k210_yolo_framework_amd import detect, draw, inference, keras_io
    from k210_yolo_framework_amd.yolonet import MODEL_DEFS
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    w = spec.init_weights(seed=1)
    ck = tmp_path / 'yolo_model.h5'
    keras_io.save_keras_weights(spec, w, ck)
    folder = tmp_path / 'pics'
    folder.mkdir()
    paths = _pictures(folder)
    net = ['--model_def', 'yolo_mobilev1', '--depth_multiplier', '0.75', '--obj_thresh', str(OBJ), '--iou_thresh', str(IOU), '--batch', '4',
           '--depth', '2']
    out1, out2 = tmp_path / 'drawn', tmp_path / 'plain'
    res = detect.cli([str(ck), str(folder), '--out_dir', str(out1), '--draw', 'True'] + net)
    printed = capsys.readouterr().out
    assert res['names'] == paths                                     # sorted folder, the text file left out
    doc = json.loads((out1 / 'detections.json').read_text())
    assert [d['path'] for d in doc] == paths
    got = [np.asarray(d['detections'], np.float32).reshape(-1, 6) for d in doc]
    assert sum(len(g) > 0 for g in got) >= 4, [len(g) for g in got]  # the threshold is low enough that most pictures have detections

    # the same pictures through inference.detect (per-picture letterbox, one Plan.run_u8, decode_py)
    h = Helper(None, 20, VOC_ANCHORS, [[224, 320]], [[7, 10], [14, 20]])
    model, _ = MODEL_DEFS['yolo_mobilev1']([224, 320, 3], 3, 20, alpha=0.75, precision='f16x2')
    model.load_weights(str(ck))
    origs = [h._read_img(p) for p in paths]
    ref = inference.detect(h, model, origs, OBJ, IOU)
    assert _assert_north_star(got, ref, 'detect vs inference.detect') == sum(len(r) for r in ref)

    # every annotated picture exists, has its source's size, and the table was printed under each path
    for p, orig in zip(paths, origs):
        f = out1 / (p.split('/')[-1].rsplit('.', 1)[0] + '_res.jpg')
        assert str(f) in res['files'] and Image.open(f).size == (orig.shape[1], orig.shape[0])
        assert p in printed
    assert printed.count('[top\tleft\tbottom\tright\tscore\tclass]') == sum(len(g) > 0 for g in got)

    # --draw False: no picture, the same JSON
    detect.cli([str(ck), str(folder), '--out_dir', str(out2), '--draw', 'False'] + net)
    assert not list(out2.glob('*.jpg')) and sorted(f.name for f in out2.iterdir()) == ['detections.json']
    assert (out2 / 'detections.json').read_text() == (out1 / 'detections.json').read_text()

    # the annotated arrays as they leave the GPU, before JPEG: the painter applied to the JSON's rows
    r = detect.run(h, model, paths, out_dir=None, draw=True, batch=4, depth=2, obj_thresh=OBJ, iou_thresh=IOU, return_arrays=True, verbose=False)
    atlas = draw.glyph_atlas()
    colours = np.asarray(h.colormap, np.uint8).reshape(-1, 3)
    checked = 0
    for i in (1, 5):                                                 # one picture of the full batch, one of the partial batch
        assert np.array_equal(r['detections'][i], got[i])
        hh, ww = origs[i].shape[:2]
        want = paint(origs[i].copy(), got[i], colours, atlas, draw.thickness_of(hh, ww), draw.magnification_of(hh))
        assert np.array_equal(r['arrays'][i], want), i
        checked += len(got[i])
    assert checked > 0
