"""CPU-side checks of `make eval` (evaluate.py, map_gpu.py): argument refusals, the ground-truth conversion, the loud failure without a
GPU, the Makefile target."""
import importlib.util
import subprocess
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import engine, evaluate

ROOT = Path(__file__).resolve().parents[1]


def test_kpu_needs_a_kmodel_and_a_kmodel_needs_kpu(capsys):
    with pytest.raises(SystemExit):
        evaluate.parse(['weights.h5', '--precision', 'kpu', '--synthetic', '8'])
    assert '--precision kpu runs a .kmodel / .kfpkg' in capsys.readouterr().err
    for mode in ('f16x2', 'f16'):
        with pytest.raises(SystemExit):
            evaluate.parse(['yolo.kmodel', '--precision', mode, '--synthetic', '8'])
        assert 'the float modes take .h5 / .npz' in capsys.readouterr().err
    a = evaluate.parse(['yolo.kfpkg', '--precision', 'kpu', '--synthetic', '8'])
    assert a.precision == 'kpu' and a.obj_thresh == 0.05 and a.voc07 == 'False' and a.synthetic_seed not in (3, 6)   # not a training seed


def test_ground_truth_rows_equal_the_developer_script():
    spec = importlib.util.spec_from_file_location('map_eval_tool', ROOT / 'tools' / 'map_eval.py')
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(11)
    for n, hw in ((0, (224, 320)), (1, (375, 500)), (7, (333, 499))):
        boxes = np.concatenate([rng.integers(0, 20, (n, 1)).astype(float), rng.uniform(0.05, 0.95, (n, 4))], 1)
        got, want = evaluate.ground_truth_rows(boxes, hw), tool.ground_truth_rows(boxes, hw)
        assert got.dtype == np.float64 and got.shape == (n, 6) and np.array_equal(got, want)


def test_map_evaluator_without_a_gpu_raises_the_librarys_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from k210_yolo_framework_amd.map_gpu import MapEvaluator
    with pytest.raises(engine.YkError, match='no CPU fallback'):
        MapEvaluator(20)
    with pytest.raises(engine.YkError, match='no CPU fallback'):
        evaluate.main(['weights.h5', '--synthetic', '8'])


def test_make_eval_expands_to_the_command_line():
    run = lambda *v: ' '.join(subprocess.run(['make', '-n', 'eval', *v], cwd=str(ROOT), capture_output=True, text=True, check=True).stdout
                              .replace('\\\n', ' ').split())
    line = run('CKPT=log/yolo_model.h5', 'SYNTHETIC=64', 'MODEL=yolo_mobilev2', 'DEPTHMUL=1.0', 'VOC07=True', 'EVALOBJ=0.1')
    assert line == ('python3 keras_eval.py log/yolo_model.h5 --train_set voc --class_num 20 --model_def yolo_mobilev2 --depth_multiplier 1.0 '
                    '--image_size 224 320 --output_size 7 10 14 20 --iou_thresh 0.5 --precision f16x2 --obj_thresh 0.1 --voc07 True --synthetic 64')
    line = run('CKPT=yolo.kmodel', 'PRECISION=kpu', 'DATASET=pet')
    assert line.endswith('--precision kpu --obj_thresh 0.05 --voc07 False --ann data/pet_img_ann.npy') and '--train_set pet' in line
    args = evaluate.parse(line.split()[2:])                                          # the target's flags are the parser's
    assert args.precision == 'kpu' and args.ann == 'data/pet_img_ann.npy' and args.iou_thresh == 0.5
    train = subprocess.run(['make', '-n', 'train', 'VALMAP=True'], cwd=str(ROOT), capture_output=True, text=True, check=True).stdout
    assert '--val_map True' in train
