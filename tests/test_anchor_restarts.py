"""Many-start anchor k-means on the CPU (datatools.anchor_inits / run_kmeans_restarts / select_anchors / make_anchor_list(restarts=)): the
numpy statement of what csrc/yk_kmeans.hip computes, the unchanged single start, and the command line."""
import importlib.util
import subprocess
from pathlib import Path

import numpy as np
import pytest

from k210_yolo_framework_amd import datatools, engine
from tests.anchor_boxes import boxes, write_ann as _ann

ROOT = Path(__file__).resolve().parents[1]


def _cli():
    spec = importlib.util.spec_from_file_location('make_anchor_list_cli', ROOT / 'make_anchor_list.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_start_zero_is_the_single_start_of_before():
    k, low, high, seed = 6, (0.1, 0.2), (0.9, 0.8), 5
    lin = np.vstack((np.linspace(0.05, 0.3, num=k), np.linspace(0.05, 0.5, num=k))).T
    rng = np.random.default_rng(seed)
    first = np.hstack((rng.uniform(low[0], high[0], (k, 1)), rng.uniform(low[1], high[1], (k, 1))))
    second = np.hstack((rng.uniform(low[0], high[0], (k, 1)), rng.uniform(low[1], high[1], (k, 1))))
    a = datatools.anchor_inits(k, 4, False, low, high, seed)
    b = datatools.anchor_inits(k, 4, True, low, high, seed)
    assert a.shape == b.shape == (4, k, 2) and a.dtype == np.float64
    assert np.array_equal(a[0], lin) and np.array_equal(a[1], first) and np.array_equal(a[2], second)    # the generator's first draw goes to start 1
    assert np.array_equal(b[0], first) and np.array_equal(b[1], second)
    assert np.array_equal(datatools.anchor_inits(k, 1, True, low, high, seed)[0], first)
    assert (a[1:, :, 0] >= low[0]).all() and (a[1:, :, 0] < high[0]).all() and (a[1:, :, 1] >= low[1]).all() and (a[1:, :, 1] < high[1]).all()


def test_one_start_on_the_cpu_gives_the_bytes_of_before(tmp_path, capsys):
    data_dir, x = _ann(tmp_path)
    for is_random, seed in ((False, None), (True, 7)):
        k = 6
        if is_random:
            rng = np.random.default_rng(seed)
            init = np.hstack((rng.uniform(0., 1., (k, 1)), rng.uniform(0., 1., (k, 1))))
        else:
            init = np.vstack((np.linspace(0.05, 0.3, num=k), np.linspace(0.05, 0.5, num=k))).T
        c, _ = datatools.run_kmeans(x, init, 10)
        want = np.array(sorted(c, key=lambda v: -v[0])).reshape(2, 3, 2)
        got = datatools.make_anchor_list('gen', is_random=is_random, seed=seed, data_dir=data_dir, restarts=1, device='cpu')
        assert got.tobytes() == want.tobytes()
        if not np.isnan(want).any():
            assert np.load(tmp_path / 'data' / 'gen_anchor.npy').tobytes() == want.tobytes()
    assert 'mean IoU' not in capsys.readouterr().out


def test_sixteen_starts_keep_the_set_with_the_highest_mean_iou(tmp_path, capsys):
    data_dir, x = _ann(tmp_path)
    inits = datatools.anchor_inits(6, 16, False, seed=3)
    runs = [datatools.run_kmeans(x, i, 10)[0] for i in inits]
    assert not any(np.isnan(c).any() for c in runs)
    ious = np.array([np.mean(1 - datatools.fake_iou_distance(x, c).min(axis=1)) for c in runs])
    assert ious.max() > ious.min()                                                   # there is something to select
    sets, score, empty = datatools.run_kmeans_restarts(x, inits, 10, 'cpu')
    assert np.array_equal(sets, np.stack(runs)) and np.array_equal(score, ious) and not empty.any()
    got = datatools.make_anchor_list('gen', is_random=False, seed=3, data_dir=data_dir, restarts=16, device='cpu', save=False)
    best = runs[int(np.argmax(ious))]
    assert got.tobytes() == np.array(sorted(best, key=lambda v: -v[0])).reshape(2, 3, 2).tobytes()
    got_iou = np.mean(1 - datatools.fake_iou_distance(x, got.reshape(-1, 2)).min(axis=1))
    assert got_iou == pytest.approx(ious.max(), abs=1e-15) and got_iou >= ious[0]
    assert f'mean IoU {ious.max():.6f} (of 16/16 starts; worst {ious.min():.6f})' in capsys.readouterr().out


def test_a_start_that_loses_a_cluster_is_flagged_where_it_happens():
    x = boxes(500, 1)
    good = datatools.anchor_inits(3, 1)[0]
    twin = good.copy()
    twin[2] = twin[0]                                                                # index 0 takes every tied box: cluster 2 is empty at once
    sets, score, empty = datatools.run_kmeans_restarts(x, np.stack([good, twin, good]), 10, 'cpu')
    assert empty.tolist() == [0, 1, 0] and np.isnan(score[1]) and np.isnan(sets[1, 2]).all() and not np.isnan(sets[1, :2]).any()
    assert np.array_equal(sets[1], datatools.run_kmeans(x, twin, 1)[0], equal_nan=True)
    assert np.isnan(datatools.run_kmeans(x, twin, 10)[0]).any()
    assert np.array_equal(sets[0], sets[2]) and score[0] == score[2] and np.array_equal(sets[0], datatools.run_kmeans(x, good, 10)[0])


def test_select_anchors_skips_flagged_starts_and_breaks_ties_low():
    c = np.arange(4 * 2 * 2, dtype=np.float64).reshape(4, 2, 2)
    r, best = datatools.select_anchors(c, np.array([0.9, 0.5, 0.7, 0.7]), np.array([3, 0, 0, 0]))
    assert r == 2 and np.array_equal(best, c[2])                                     # 0 has the highest score but is flagged; 2 and 3 tie
    r, best = datatools.select_anchors(c, np.array([np.nan, 0.5, np.nan, 0.6]), np.array([1, 0, 2, 0]))
    assert r == 3 and np.array_equal(best, c[3])
    c[:, 1] = np.nan
    r, best = datatools.select_anchors(c, np.full(4, np.nan), np.array([1, 1, 4, 2]))
    assert np.isnan(best).any() and best.shape == (2, 2)


def test_all_starts_flagged_prints_the_reference_error_and_saves_nothing(tmp_path, capsys):
    data_dir, _ = _ann(tmp_path)
    # every centroid is drawn from a point: all start equal, index 0 takes every box
    got = datatools.make_anchor_list('gen', is_random=True, low=(0.3, 0.3), high=(0.3, 0.3), seed=0, data_dir=data_dir, restarts=3, device='cpu')
    assert np.isnan(got).any() and '[ERROR] Result have NaN value please Rerun!' in capsys.readouterr().out
    assert not (tmp_path / 'data' / 'gen_anchor.npy').exists()


def test_refusals_name_the_argument(tmp_path):
    data_dir, x = _ann(tmp_path)
    with pytest.raises(ValueError, match='device'):
        datatools.make_anchor_list('gen', data_dir=data_dir, device='tpu')
    with pytest.raises(ValueError, match='restarts'):
        datatools.make_anchor_list('gen', data_dir=data_dir, restarts=0)
    bad = x.copy()
    bad[5, 1] = 0.0
    with pytest.raises(ValueError, match='x holds a box'):
        datatools.run_kmeans_restarts(bad, datatools.anchor_inits(3, 2), 10, 'cpu')
    with pytest.raises(ValueError, match='inits of shape'):
        datatools.run_kmeans_restarts(x, np.zeros((3, 2, 3)), 10, 'cpu')


def test_cli_flags_parse_and_reach_make_anchor_list(tmp_path, capsys):
    cli = _cli()
    a = cli.parse(['voc'])
    assert (a.device, a.restarts, a.seed, a.data_dir) == ('cpu', 1, None, 'data')
    a = cli.parse(['pet', '--device', 'gpu', '--restarts', '256', '--seed', '4'])
    assert (a.train_set, a.device, a.restarts, a.seed) == ('pet', 'gpu', 256, 4)
    for bad in (['voc', '--device', 'tpu'], ['voc', '--restarts', '0']):
        with pytest.raises(SystemExit):
            cli.parse(bad)
    capsys.readouterr()
    data_dir, _ = _ann(tmp_path)
    got = cli.main(['gen', '--is_random', 'True', '--seed', '2', '--restarts', '4', '--data_dir', data_dir])
    want = datatools.make_anchor_list('gen', is_random=True, seed=2, data_dir=data_dir, restarts=4, save=False)
    out = capsys.readouterr().out
    assert got.tobytes() == want.tobytes() and 'of 4/4 starts' in out and '[NOTE] Now anchors are' in out


def test_cli_device_gpu_without_a_device_fails_loudly(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)                   # what a machine without a device answers
    data_dir, x = _ann(tmp_path)
    with pytest.raises(engine.YkError, match='no CPU fallback'):
        _cli().main(['gen', '--device', 'gpu', '--restarts', '4', '--data_dir', data_dir])
    with pytest.raises(engine.YkError, match='no CPU fallback'):
        datatools.run_kmeans_gpu(x, datatools.anchor_inits(6, 2))
    assert not (tmp_path / 'data' / 'gen_anchor.npy').exists()


def test_make_anchors_expands_to_the_command_line():
    run = lambda *v: ' '.join(subprocess.run(['make', '-n', 'anchors', *v], cwd=str(ROOT), capture_output=True, text=True, check=True).stdout
                              .replace('\\\n', ' ').split())
    line = run()
    assert line == ('python3 ./make_anchor_list.py voc --max_iters 10 --is_random True --in_hw 224 320 --out_hw 7 10 14 20 --anchor_num 3 '
                    '--low 0.0 0.0 --high 1.0 1.0 --device cpu --restarts 1')
    a = _cli().parse(line.split()[2:])
    assert (a.device, a.restarts, a.seed) == ('cpu', 1, None)
    line = run('ANCDEVICE=gpu', 'RESTARTS=256', 'ANCSEED=3', 'DATASET=pet')
    assert line.endswith('--device gpu --restarts 256 --seed 3') and ' pet ' in line
    a = _cli().parse(line.split()[2:])
    assert (a.train_set, a.device, a.restarts, a.seed) == ('pet', 'gpu', 256, 3)
