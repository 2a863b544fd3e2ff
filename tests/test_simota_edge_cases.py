"""tests/simota_edge_cases.py checked on its own, on the CPU: every case reaches the path of csrc/yk_ota.hip it is named for - read from
simota.assign's `detail` - every random case has the rule's margin above 1e-9 and every crafted tie is bit-equal in the rule with the
decisions beside it more than 1e-9 apart; `detail` changes no result; and yk_assign_simota_f32 refuses by name, before the device, what
the GPU file must not launch."""
import ctypes as C
import math

import numpy as np
import pytest

from k210_yolo_framework_amd import simota
from tests import simota_cases
from tests import simota_edge_cases as ec

LDS_CANDS, MAX_TOPK = 6144, 32                                  # YK_OTA_LDS_CANDS, YK_OTA_MAX_TOPK


def records(name):
    return ec.rule(name)[4]


def owners_by_layer(name):
    cfg = ec.case(name)['cfg']
    return sorted({ec.layer_of(cfg, j) for r in records(name) for j, o in r['owner'].items() if o == r['g']})


def most_contenders(name):
    return max([len(v) + 1 for r in records(name) for v in r.get('rivals', {}).values()] + [0])


@pytest.mark.parametrize('name', sorted(ec.BUILDERS))
def test_every_decision_is_exact_or_more_than_1e9_apart(name):
    c = ec.case(name)
    labels, npos, status, margin, detail = ec.rule(name)
    assert len(detail) > 0 and int(npos.sum()) > 0
    if c['ties']:
        assert ec.nonzero_gap(detail, c['boxes']) > 1e-9                         # (a tie inside a selection does not show in the margin)
    else:
        assert margin > 1e-9, margin
        assert ec.nonzero_gap(detail, c['boxes']) >= margin
    for p in c['preds']:
        assert p.dtype == np.float32 and np.isfinite(p).all()


@pytest.mark.parametrize('case', [c for c in simota_cases.CASES if c['id'] != '76x76-past-the-LDS-strip-of-6144'], ids=lambda c: c['id'])
def test_detail_changes_no_result_and_says_what_was_written(case):
    cfg, preds, boxes, first, opts = simota_cases.build(case)
    want, detail = simota.assign(preds, boxes, first, cfg, **opts), []
    got = simota.assign(preds, boxes, first, cfg, detail=detail, **opts)
    assert all(np.array_equal(g, w) for g, w in zip(got[0], want[0])) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    owned = np.zeros(len(first) - 1, np.int64)
    for r in detail:
        assert r['k'] == len(r['j']) == min(r['E'], max(1, math.floor(r['S']))) and len(r['el']) == r['E'] and sorted(r['rivals']) == sorted(r['j'])
        owned[r['image']] += sum(o == r['g'] for o in r['owner'].values())
    assert owned.tolist() == got[1].tolist()


def test_many_rounds_reach_half_the_selection_table_and_candidates_are_contested():
    for name in ('rounds-topk-10', 'rounds-topk-32-radius-16'):
        assert most_contenders(name) >= 2 and owners_by_layer(name) == [0, 1]
    assert max(r['k'] for r in records('rounds-topk-10')) >= 6 and min(r['E'] for r in records('rounds-topk-10')) > 10
    assert max(r['k'] for r in records('rounds-topk-32-radius-16')) >= 16
    assert all(r['E'] == 720 for r in records('rounds-topk-32-radius-16'))       # radius 16: every candidate, 32 rounds of the first search


@pytest.mark.parametrize('topk, k', [(32, 8), (3, 3)])
def test_k_equals_e(topk, k):
    (r,) = records(f'k-equals-E-topk-{topk}')
    assert r['E'] == 8 and r['S'] == float(k) and r['k'] == k and (r['iou'] == 1.0).all() and len(set(r['cost'].tolist())) == 1
    assert r['j'] == list(range(72, 72 + k))                                     # the lowest j win
    assert all(r['in_box']) and all(r['in_ctr'])


@pytest.mark.parametrize('name, partners, taken', [
    ('tie-in-one-wave-topk-1', [119, 120], [119]), ('tie-in-one-wave-topk-4', [119, 120], [119, 120, 103]),
    ('tie-across-waves-topk-1', [119, 120, 135, 136], [119]), ('tie-across-waves-topk-4', [119, 120, 135, 136], [119, 120, 135]),
    ('tie-of-one-lane-j-and-j+256-topk-1', [37, 293], [37]), ('tie-of-one-lane-j-and-j+256-topk-4', [37, 293], [37, 293])])
def test_tie_levels(name, partners, taken):
    (r,) = records(name)
    cost, iou = dict(zip(r['el'].tolist(), r['cost'].tolist())), dict(zip(r['el'].tolist(), r['iou'].tolist()))
    assert len({cost[j] for j in partners}) == 1 and len({iou[j] for j in partners}) == 1       # bit-equal
    assert cost[partners[0]] == min(cost.values()) and sorted(j for j in cost if cost[j] == cost[partners[0]]) == partners
    assert r['j'] == taken and r['k'] == len(taken)
    if len(taken) == 3:                                                          # the third round is decided among tied costs as well
        assert sum(v == cost[taken[2]] for v in cost.values()) >= 2 and taken[2] == min(j for j in cost if cost[j] == cost[taken[2]] and j not in taken[:2])
    # wave = j // 64 % 4, lane = j % 256
    waves = {j // 64 % 4 for j in partners}
    assert len(waves) == (2 if 'across' in name else 1) and (partners[1] - partners[0] == 256) == ('one-lane' in name)


@pytest.mark.parametrize('name, cls', [('cross-box-tie-class-0-first', 0), ('cross-box-tie-class-1-first', 1)])
def test_cross_box_tie_of_different_rows(name, cls):
    c, (a, b) = ec.case(name), records(name)
    assert not np.array_equal(c['boxes'][0], c['boxes'][1]) and a['j'] == b['j'] and a['j_cost'] == b['j_cost'] and len(a['j']) == 2
    assert all(o == 0 for o in a['owner'].values()) and all(v == [1] for v in a['rivals'].values())
    labels = ec.rule(name)[0][0].reshape(-1, 7)
    assert labels[a['j'], 5 + cls].tolist() == [1, 1] and labels[a['j'], 6 - cls].tolist() == [0, 0]


def test_negative_costs():
    (r,) = records('negative-cost-in-a-selection-of-2')
    assert r['k'] == 2 and r['j_cost'][0] == 3 * -math.log(1 + 1e-8) < 0 < r['j_cost'][1]
    a, b = records('negative-costs-contend')
    assert a['j'] == b['j'] == [0] and b['j_cost'][0] < a['j_cost'][0] < 0 and a['j_cost'][0] - b['j_cost'][0] > 1e-9 and a['owner'][0] == 1
    boxes, label = ec.case('negative-costs-contend')['boxes'], ec.rule('negative-costs-contend')[0][0].reshape(-1)
    assert np.float32(boxes[0, 1]) != np.float32(boxes[1, 1]) and label[0] == np.float32(boxes[1, 1])     # the labels name the owner
    a, b = records('negative-costs-contend-bit-equal')
    assert a['j'] == b['j'] == [0] and a['j_cost'] == b['j_cost'] and a['j_cost'][0] < 0 and a['owner'][0] == 0
    boxes = ec.case('negative-costs-contend-bit-equal')['boxes']
    assert not np.array_equal(boxes[0], boxes[1])


def test_strip_cases_sit_on_both_sides_of_the_switch():
    sizes = {n: ec.n_candidates(ec.case(n)['cfg']) for n in ec.BUILDERS if n.startswith('N-')}
    assert sorted(sizes.values()) == [LDS_CANDS, LDS_CANDS + 1, LDS_CANDS + 3, LDS_CANDS + 3]
    for name in sizes:
        if sizes[name] == LDS_CANDS + 3:
            c = ec.case(name)
            assert np.diff(c['first']).tolist() == [2, 0, 3] and [r['image'] for r in records(name)] == [0, 0, 2, 2, 2]
            assert c['opts'].get('max_boxes', 64) >= 3 and ec.rule(name)[2] == simota.STATUS_CLEAN


@pytest.mark.parametrize('name, C', [('four-ragged-layers-C3', 3), ('four-ragged-layers-C30', 30)])
def test_four_ragged_layers_have_owners_in_every_layer_of_every_image(name, C):
    c = ec.case(name)
    sizes = [h * w * len(a) for (h, w), a in zip(c['cfg']['out_hw'], c['cfg']['anchors'])]
    assert [len(a) for a in c['cfg']['anchors']] == [1, 8, 3, 2] and all(h % 2 and w % 2 for h, w in c['cfg']['out_hw'])
    tc, bounds = ec.prep_tile(C), np.cumsum(sizes)[:-1]
    assert tc == (256 if C == 3 else 193) and all(b % tc for b in bounds) and sum(sizes) > 256      # every boundary is inside a tile
    assert owners_by_layer(name) == [0, 1, 2, 3]
    labels = ec.rule(name)[0]
    assert all((l[s, ..., 4] > 0).any() for l in labels[1:] for s in range(3)) and len(c['first']) == 4


def test_tile_sizes():
    want = {22: 256, 23: 250, 600: 9, 2999: 2, 4096: 1}
    for C, tc in want.items():
        c = ec.case(f'tile-C{C}')
        assert c['cfg']['class_num'] == C and ec.prep_tile(C) == tc and ec.n_candidates(c['cfg']) == 12
        if C >= 600:
            assert c['boxes'][:, 0].tolist() == [0, C - 1]
    assert ec.case('tile-C22')['cfg']['out_hw'] == ec.case('tile-C23')['cfg']['out_hw']                      # one shape either side of 256


def test_large_cases():
    c = ec.case('clear-grid-stride-5.8M')
    assert sum(p.size for p in c['preds']) > 4096 * 256 * 4 and sorted({r['image'] for r in records('clear-grid-stride-5.8M')}) == [0, 25, 51]
    c = ec.case('n-65535')
    assert len(c['first']) == 65536 and sorted(r['image'] for r in records('n-65535')) == [0, 30000, 65534]
    assert ec.rule('n-65535')[1].sum() == 3


def test_hostile_offsets_are_clamped_by_the_rule_as_by_the_kernel():
    # [0, 2, 1, 9] on 5 rows: image 0 rows 0 .. 1, image 1 none (descending), image 2 rows 1 .. 4 (the end clamped to the row count)
    assert [(r['image'], r['g']) for r in records('offsets-descending-then-past-the-end')] == [(0, 0), (0, 1), (2, 1), (2, 2), (2, 3), (2, 4)]
    assert [(r['image'], r['g']) for r in records('offsets-negative')] == [(0, 0), (0, 1), (1, 2), (1, 3), (1, 4)]
    # a start past the end leaves nothing: b1 is clamped to the row count, and b1 <= b0 is skipped
    c = ec.case('offsets-negative')
    labels, npos, status, _ = simota.assign(c['preds'], c['boxes'], [9, 9, 5], c['cfg'])
    assert npos.tolist() == [0, 0] and status == simota.STATUS_CLEAN and not any(l.any() for l in labels)
    labels, npos, status, _ = simota.assign(c['preds'], c['boxes'], [7, 2, 100], c['cfg'])
    assert npos[0] == 0 and npos[1] > 0


def test_status_cases():
    assert ec.rule('status-invalid-in-images-1-and-2')[2] == 3
    assert [r['g'] for r in records('status-invalid-in-images-1-and-2')] == [0, 1, 2, 5, 7]
    assert ec.rule('status-overflow-in-image-0-invalid-in-image-1')[2] == 2
    assert [r['g'] for r in records('status-overflow-in-image-0-invalid-in-image-1')] == [0, 1, 3]
    labels, npos, status, _, detail = ec.rule('status-hostile-values')
    assert status == 2 and [r['g'] for r in detail] == ec.HOSTILE_VALID
    assert not any(np.isnan(l).any() for l in labels)                           # a NaN width is clipped to 1e-8 (C's fmax), not written
    boxes, written = ec.case('status-hostile-values')['boxes'], {}
    for r in detail:
        for j, o in r['owner'].items():
            if o == r['g']:
                l, jl = ec.layer_of(ec.case('status-hostile-values')['cfg'], j), j - (0 if j < 18 else 18)
                written[r['g']] = labels[l][0].reshape(-1, 8)[jl]
    f = np.float32
    assert written[8][0] == f(1e-8) and written[9][2] == f(1e-8) and written[10][2] == f(1e-8) and written[11][2] == 1
    assert written[12][2] == f(1e-8) and written[13][3] == f(1e-8) and written[14][2] == 1 and written[15][3] == f(1e-8)
    assert written[16][2] == f(1e-8) and written[17][3] == 1 and written[0][5] == 1 and written[1][7] == 1
    assert np.isnan(boxes[12, 3]) and np.isnan(boxes[13, 4])


def test_contention_of_256_boxes():
    c = ec.case('contention-256-boxes')
    assert c['opts']['max_boxes'] == 256 and np.diff(c['first']).tolist() == [256, 3] and ec.n_candidates(c['cfg']) == 48
    assert most_contenders('contention-256-boxes') >= 8 and len(records('contention-256-boxes')) == 259


def test_degenerate_decodes():
    c, detail = ec.case('degenerate-decodes'), records('degenerate-decodes')
    tw, th = c['preds'][0][..., 2], c['preds'][0][..., 3]
    assert (tw[0] == -800).all() and {-800., 90., 800.} <= set(tw[1].ravel().tolist()) and {-800., 90., 800.} <= set(th[1].ravel().tolist())
    assert ((tw[1] == 90) & (th[1] == 800)).any() and ((tw[1] == -800) & (th[1] == 800)).any()         # U infinite, and 0 * inf
    for r in detail[:2]:
        assert r['S'] == 0.0 and r['k'] == 1 and not r['iou'].any() and r['E'] > 32                    # every IoU key equal
    assert detail[0]['j'] == detail[1]['j'] and detail[0]['j_cost'] == detail[1]['j_cost'] and detail[0]['owner'][detail[0]['j'][0]] == 0
    assert all(np.isfinite(r['cost']).all() for r in detail)


@pytest.mark.parametrize('what, names', [
    (dict(n=65536), 'n = 65536'), (dict(out_h=4096, out_w=4097), 'more than 2\\^24 candidates'), (dict(anchor0=0), 'cfg->anchor_num\\[0\\] = 0'),
    (dict(anchor0=9), 'cfg->anchor_num\\[0\\] = 9'), (dict(n_layers=0), 'cfg->n_layers = 0'), (dict(n_layers=5), 'cfg->n_layers = 5'),
    (dict(class_num=4097), 'cfg->class_num = 4097'), (dict(misaligned=True), 'a misaligned pointer')])
def test_refused_by_name_before_the_device(what, names):
    from k210_yolo_framework_amd import engine
    cfg = engine.make_ota_cfg(dict(out_hw=[(1, 1)], anchors=[[(.5, .5)]], class_num=1))
    for field in ('n_layers', 'class_num'):
        if field in what:
            setattr(cfg, field, what[field])
    if 'out_h' in what:
        cfg.out_h[0], cfg.out_w[0] = what['out_h'], what['out_w']
    if 'anchor0' in what:
        cfg.anchor_num[0] = what['anchor0']
    n = what.get('n', 1)
    if what.get('misaligned'):
        # host memory standing in for every buffer: the alignment check comes before the device and before anything is read
        room = (C.c_double * 64)()
        at = C.addressof(room)
        ptrs = (C.c_void_p * 4)(at + 64, 0, 0, 0)
        with pytest.raises(engine.YkError, match='yk_assign_simota_f32: ' + names):
            engine.call('yk_assign_simota_f32', C.byref(cfg), C.c_void_p(at), 1, C.c_void_p(at + 128), n, ptrs, C.c_void_p(at + 192 + 2),
                        C.c_void_p(at + 256), C.c_void_p(at + 260), C.c_void_p(at + 320), 1 << 20, None)
        return
    with pytest.raises(engine.YkError, match='yk_assign_simota_f32: ' + names):
        engine.call('yk_assign_simota_f32', C.byref(cfg), None, 0, None, n, None, None, None, None, None, 0, None)
