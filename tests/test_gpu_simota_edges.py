"""csrc/yk_ota.hip's four launches held to simota.assign on the cases of tests/simota_edge_cases.py - many selection rounds, k == E, ties
inside a wave, across waves and between one lane's own entries, cross-box ties, negative costs, both sides of the LDS strip and strips of
several images, four ragged layers, every tile size of ota_prep, ota_clear off its alignment and past one grid, n = 65535, hostile offsets,
every kind of invalid row, 256 boxes on 48 candidates, degenerate decodes - by np.array_equal on every grid, npos and status: no tolerance
enters.  A second call into buffers full of 7.0 / -3 gives the same bytes; a workspace of exactly the asked size inside 0xFF bytes keeps
its neighbours; and the device's own results have the rule's symmetries.  tests/test_simota_edge_cases.py proves on the CPU that every case
reaches what it is here for."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import simota_edge_cases as ec

pytestmark = pytest.mark.gpu


def upload(c):
    import torch
    return [torch.from_numpy(p).cuda() for p in c['preds']]


def on_engine(c, out=None, stream=None, dev=None):
    """engine.assign_simota on a case -> (views, npos, status) on the device.  The box buffer has spare NaN rows past the last offset, as
    in a captured step."""
    from k210_yolo_framework_amd import engine
    padded = np.concatenate([c['boxes'], np.full((3, 5), np.nan)])
    return engine.assign_simota(dev if dev is not None else upload(c), padded, c['first'], engine.make_ota_cfg(c['cfg'], **c['opts']), out=out, stream=stream)


def same_as_rule(got, want):
    views, npos, status = got
    labels, wnpos, wstatus = want[:3]
    for l, (g, w) in enumerate(zip(views, labels)):
        g = g.cpu().numpy()
        assert np.array_equal(g, w), (l, np.argwhere(g != w)[:5])
    assert npos.cpu().numpy().tolist() == wnpos.tolist() and int(status.item()) == wstatus


@functools.lru_cache(maxsize=None)
def first_call(name):
    return on_engine(ec.case(name))


@pytest.mark.parametrize('name', ec.ENGINE)
def test_every_case_equals_the_rule_and_two_calls_give_the_same_bytes(name):
    import torch
    c = ec.case(name)
    got = first_call(name)
    same_as_rule(got, ec.rule(name))
    views, npos, status = got
    out = (torch.full((sum(v.numel() for v in views),), 7.0, device='cuda'), torch.full((len(c['first']) - 1,), -3, dtype=torch.int32, device='cuda'),
           torch.zeros(1, dtype=torch.int32, device='cuda'))
    again, anpos, astatus = on_engine(c, out=out)
    assert all(torch.equal(a, g) for a, g in zip(again, views)) and torch.equal(anpos, npos) and torch.equal(astatus, status)


@pytest.mark.parametrize('name', ec.LARGE)
def test_large_cases_compared_on_the_device(name):
    """5.8M floats of grids (ota_clear's grid-stride loop) and 65535 images (the largest gridDim.y): one call into buffers full of 7.0 / -3,
    compared whole against the uploaded expectation."""
    import torch
    c = ec.case(name)
    labels, npos, status = ec.rule(name)[:3]
    flat = torch.full((sum(l.size for l in labels),), 7.0, device='cuda')
    out = (flat, torch.full((len(npos),), -3, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'))
    views, gnpos, gstatus = on_engine(c, out=out)
    for v, l in zip(views, labels):
        assert torch.equal(v, torch.from_numpy(l).cuda())
    assert torch.equal(gnpos, torch.from_numpy(npos).cuda()) and int(gstatus.item()) == status


def test_no_image_launches_nothing_and_leaves_the_status_clean():
    import torch
    from k210_yolo_framework_amd import engine, simota
    cfg = ec.case('clear-mid')['cfg']
    dev = [torch.zeros((0, h, w, len(a), 5 + cfg['class_num']), device='cuda') for (h, w), a in zip(cfg['out_hw'], cfg['anchors'])]
    views, npos, status = engine.assign_simota(dev, np.zeros((0, 5)), np.zeros(1, np.int32), engine.make_ota_cfg(cfg))
    assert [v.numel() for v in views] == [0, 0] and npos.numel() == 0 and int(status.item()) == simota.STATUS_CLEAN


@pytest.mark.parametrize('name', ['clear-1x1', 'clear-mid'])
@pytest.mark.parametrize('lead', [1, 2, 3])
def test_clear_off_its_alignment_keeps_its_neighbours(name, lead):
    """ota_clear's head, a count below head + 4 (6 floats: no or one 16-byte store) and its tail, through out= views that start `lead`
    floats into a buffer of 7.0."""
    import torch
    c, labels = ec.case(name), ec.rule(name)[0]
    total = sum(l.size for l in labels)
    room = torch.full((total + 8,), 7.0, device='cuda')
    assert room.data_ptr() % 16 == 0
    out = (room[lead:lead + total], torch.full((len(c['first']) - 1,), -3, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda'))
    same_as_rule(on_engine(c, out=out), ec.rule(name))
    host = room.cpu().numpy()
    assert (host[:lead] == 7.0).all() and (host[lead + total:] == 7.0).all()
    assert np.array_equal(host[lead:lead + total], np.concatenate([l.reshape(-1) for l in labels]))


def direct(c, short=0):
    """yk_assign_simota_f32 itself with n_boxes = the row count, the workspace exactly yk_simota_workspace_bytes long inside a larger buffer
    of 0xFF bytes, 8 bytes past a 16-byte boundary, the outputs full of 7.0 / -3 -> (flat labels, npos, status, the buffer, offset, bytes)"""
    import torch
    from k210_yolo_framework_amd import engine
    cfg, n = engine.make_ota_cfg(c['cfg'], **c['opts']), len(c['first']) - 1
    need = C.c_size_t(0)
    engine.call('yk_simota_workspace_bytes', C.byref(cfg), n, int(cfg.max_boxes), C.byref(need))
    room = torch.full((need.value + 1024,), 0xFF, dtype=torch.uint8, device='cuda')
    at = 256 + (8 - room.data_ptr() % 16) % 16
    work = room[at:at + need.value]
    assert work.data_ptr() % 16 == 8
    dev, boxes, first = upload(c), torch.from_numpy(c['boxes']).cuda(), torch.from_numpy(np.asarray(c['first'], np.int32)).cuda()
    out = (torch.full((sum(p.numel() for p in dev),), 7.0, device='cuda'), torch.full((n,), -3, dtype=torch.int32, device='cuda'),
           torch.zeros(1, dtype=torch.int32, device='cuda'))
    ptrs = (C.c_void_p * engine.YK_MAX_LAYERS)(*[p.data_ptr() for p in dev])
    engine.call('yk_assign_simota_f32', C.byref(cfg), boxes, int(boxes.shape[0]), first, n, ptrs, out[0], out[1], out[2], work, need.value - short, None)
    torch.cuda.synchronize()
    return out + (room, at, need.value)


def views_of(flat, labels):
    views, at = [], 0
    for l in labels:
        views.append(flat[at:at + l.size].view(l.shape))
        at += l.size
    return views


@pytest.mark.parametrize('name', ec.DIRECT)
def test_direct_call_equals_the_rule_and_stays_inside_its_workspace(name):
    c, want = ec.case(name), ec.rule(name)
    flat, npos, status, room, at, nbytes = direct(c)
    same_as_rule((views_of(flat, want[0]), npos, status), want)
    host = room.cpu().numpy()
    assert (host[:at] == 0xFF).all() and (host[at + nbytes:] == 0xFF).all()
    if name.startswith('N-'):
        assert ec.n_candidates(c['cfg']) > 6144 and nbytes > 3 * c['opts'].get('max_boxes', 64) * 6147 * 8      # the strips are in it


def test_a_workspace_one_byte_short_is_refused_by_name():
    from k210_yolo_framework_amd import engine
    with pytest.raises(engine.YkError, match='yk_assign_simota_f32: work_bytes = '):
        direct(ec.case('N-6147-strips-of-3-images-max_boxes-3'), short=1)


def test_large_small_large_on_one_stream_and_a_side_stream():
    """The engine's workspace only grows: the small call runs in the large call's stale cells, and the second large call in both's."""
    import torch
    big, small = 'N-6147-strips-of-3-images-max_boxes-64', 'clear-1x1'
    for name in (big, small, big, 'four-ragged-layers-C30'):
        same_as_rule(on_engine(ec.case(name)), ec.rule(name))
    side = torch.cuda.Stream()
    for name in (big, 'contention-256-boxes'):
        dev = upload(ec.case(name))
        side.wait_stream(torch.cuda.current_stream())
        got = on_engine(ec.case(name), stream=side, dev=dev)
        side.synchronize()
        same_as_rule(got, ec.rule(name))


@pytest.mark.parametrize('name', ['rounds-topk-10', 'four-ragged-layers-C3', 'clear-mid', 'N-6145-the-first-on-the-strip'])
def test_permuting_an_images_rows_changes_nothing(name):
    """(cases without cross-box ties: there the row order is the tie-break)"""
    import torch
    views, npos, status = first_call(name)
    moved, mnpos, mstatus = on_engine(ec.permuted(ec.case(name)))
    assert all(torch.equal(m, v) for m, v in zip(moved, views)) and torch.equal(mnpos, npos) and torch.equal(mstatus, status)


@pytest.mark.parametrize('name', ['rounds-topk-32-radius-16', 'four-ragged-layers-C30', 'cross-box-tie-class-1-first', 'N-6144-the-last-in-LDS'])
def test_appending_an_image_changes_no_earlier_image(name):
    import torch
    views, npos, _ = first_call(name)
    more, mnpos, _ = on_engine(ec.appended(ec.case(name)))
    n = npos.numel()
    assert mnpos.numel() == n + 1 and all(torch.equal(m[:n], v) for m, v in zip(more, views)) and torch.equal(mnpos[:n], npos)
    assert int(mnpos[n]) > 0
