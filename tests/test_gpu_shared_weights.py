"""Plans built from the same weights read one device copy of the packed weights (csrc/yk_wstore.h): what must stay true around it.

The network is the smallest with every kernel family - yolo_mobilev1 0.5 at 64x96, max_batch 2 - in both precisions and both schedules
(the f16 builder has one schedule; it is run under both names).  YK_SHARE_WEIGHTS=0 at plan creation gives a plan its own copies: the
twin every shared plan is compared with, bit for bit.

Memory bounds.  `packed_bytes` is a LOWER bound of what a plan packs, from the spec alone: every conv weight is stored as an fp16 pair
(f16x2: 4 bytes) or one fp16 (f16: 2 bytes), padding, depthwise tables and BatchNorm tables not counted.  A second shared plan must
cost less device memory than a second private one by more than half of that.  GRANULE is the block size in which the runtime hands
small device allocations back to the driver (2 MiB): once every plan is closed, free memory must be back within one such block of
where it started."""
import contextlib
import os
import threading

import numpy as np
import pytest
import torch

from k210_yolo_framework_amd import engine, netspec as ns

pytestmark = pytest.mark.gpu

B = 2
HW = (64, 96)
GRANULE = 2 << 20
CASES = [('f16x2', 'throughput'), ('f16x2', 'latency'), ('f16', 'throughput'), ('f16', 'latency')]
_ids = [f'{p}-{s}' for p, s in CASES]
_cache = {}


def _net():
    if 'net' not in _cache:
        spec = ns.yolo_mobilev1((*HW, 3), 3, 20, alpha=0.5)
        w = spec.init_weights(seed=3)
        last = [l for l in spec.layers if l.kind == 'conv'][-1].name + '/kernel'
        w2 = dict(w)
        k = w[last].copy()
        k.flat[k.size // 2] += 0.5                                           # one element of the last conv
        w2[last] = k
        g = torch.Generator(device='cuda').manual_seed(5)
        frames = torch.randint(0, 256, (40, B, *HW, 3), dtype=torch.uint8, device='cuda', generator=g)
        _cache['net'] = (spec, w, w2, frames)
    return _cache['net']


def packed_bytes(spec, precision):
    return sum(int(np.prod(l.kernel_shape)) for l in spec.layers if l.kind == 'conv') * (4 if precision == 'f16x2' else 2)


@contextlib.contextmanager
def _private():
    old = os.environ.get('YK_SHARE_WEIGHTS')
    os.environ['YK_SHARE_WEIGHTS'] = '0'
    try:
        yield
    finally:
        if old is None:
            del os.environ['YK_SHARE_WEIGHTS']
        else:
            os.environ['YK_SHARE_WEIGHTS'] = old


def _plan(weights, precision, schedule, private=False):
    spec = _net()[0]
    with (_private() if private else contextlib.nullcontext()):
        return engine.Plan(spec, weights, max_batch=B, precision=precision, schedule=schedule)


def _run(plan, frames):
    plan.run_u8(frames)
    plan.check()
    return [o.cpu().numpy().copy() for o in plan.outputs()]


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _reference(weights_key, precision, schedule, step=0):
    """outputs of a private plan for frames[step]: computed once per (weights, precision, schedule, step), never changed"""
    key = (weights_key, precision, schedule, step)
    if key not in _cache:
        spec, w, w2, frames = _net()
        with _plan(w if weights_key == 'w' else w2, precision, schedule, private=True) as p:
            _cache[key] = _run(p, frames[step])
    return _cache[key]


@pytest.mark.parametrize('precision,schedule', CASES, ids=_ids)
def test_second_plan_shares_and_matches_private(precision, schedule):
    spec, w, _, frames = _net()
    ref = _reference('w', precision, schedule)
    with _plan(w, precision, schedule) as a:
        more = []

        def cost(private):
            """the largest of three consecutive creations: the runtime serves small allocations from the 2 MiB blocks it has cached before it asks
            the driver for more, so after other tests a single creation can read low; the plans stay alive, so the cached room runs out"""
            deltas = []
            for _ in range(3):
                m = _free()
                more.append(_plan(w, precision, schedule, private=private))
                deltas.append(m - _free())
            return max(deltas)

        try:
            shared_cost, private_cost = cost(False), cost(True)
            pk = packed_bytes(spec, precision)
            print(f'{precision}-{schedule}: second plan costs {shared_cost} bytes shared, {private_cost} private; packed weights >= {pk}')
            oa = _run(a, frames[0])
            assert _same(oa, ref) and any(np.abs(o).max() > 0 for o in oa)
            for plan in more:
                assert _same(_run(plan, frames[0]), oa)
            assert shared_cost < private_cost - pk / 2, (shared_cost, private_cost, pk)
        finally:
            for plan in more:
                plan.close()


@pytest.mark.parametrize('precision,schedule', CASES, ids=_ids)
def test_lifetime_entry_outlives_its_first_plan_and_is_rebuilt(precision, schedule):
    _, w, _, frames = _net()
    ref = _reference('w', precision, schedule)
    a = _plan(w, precision, schedule)
    b = _plan(w, precision, schedule)
    assert _same(_run(a, frames[0]), ref)
    a.close()
    filler = torch.full((8 << 20,), 0x7f7f7f7f, dtype=torch.int32, device='cuda')   # what a freed buffer would soon hold
    assert _same(_run(b, frames[0]), ref)
    b.close()
    del filler
    with _plan(w, precision, schedule) as c:                                         # the entry was freed; this one builds it again
        assert _same(_run(c, frames[0]), ref)


@pytest.mark.parametrize('precision,schedule', CASES, ids=_ids)
def test_one_changed_weight_is_another_entry(precision, schedule):
    _, w, w2, frames = _net()
    ref, ref2 = _reference('w', precision, schedule), _reference('w2', precision, schedule)
    assert not _same(ref, ref2)
    with _plan(w, precision, schedule) as a, _plan(w2, precision, schedule) as b:
        oa, ob = _run(a, frames[0]), _run(b, frames[0])
        assert _same(oa, ref) and _same(ob, ref2) and not _same(oa, ob)


def test_precisions_and_schedules_do_not_alias():
    _, w, _, frames = _net()
    plans = [_plan(w, p, s) for p, s in CASES]                                       # all alive at once, from the same weights
    try:
        for plan, (p, s) in zip(plans, CASES):
            assert _same(_run(plan, frames[0]), _reference('w', p, s)), (p, s)
    finally:
        for plan in plans:
            plan.close()


@pytest.mark.parametrize('precision,schedule', CASES, ids=_ids)
def test_two_shared_plans_on_two_streams(precision, schedule):
    _, w, _, frames = _net()
    steps = 20
    alone = []
    with _plan(w, precision, schedule, private=True) as p:
        for i in range(2 * steps):
            alone.append(_run(p, frames[i]))
    a, b = _plan(w, precision, schedule), _plan(w, precision, schedule)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    got_a, got_b = [], []
    try:
        torch.cuda.synchronize()
        for i in range(steps):
            with torch.cuda.stream(sa):
                a.run_u8(frames[i], stream=sa)
                got_a.append([o.clone() for o in a.outputs()])
            with torch.cuda.stream(sb):
                b.run_u8(frames[steps + i], stream=sb)
                got_b.append([o.clone() for o in b.outputs()])
        a.check()
        b.check()
        torch.cuda.synchronize()
        for i in range(steps):
            assert _same([o.cpu().numpy() for o in got_a[i]], alone[i]), i
            assert _same([o.cpu().numpy() for o in got_b[i]], alone[steps + i]), i
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('precision,schedule', CASES, ids=_ids)
def test_four_threads_make_one_entry_and_nothing_leaks(precision, schedule):
    spec, w, _, frames = _net()
    ref = _reference('w', precision, schedule)
    pk = packed_bytes(spec, precision)
    _plan(w, precision, schedule).close()                                            # code objects loaded, allocator warm
    held, deltas = [], []
    for _ in range(3):                                                               # (the largest of three, as in the first test)
        m = _free()
        held.append(_plan(w, precision, schedule, private=True))
        deltas.append(m - _free())
    private_cost = max(deltas)
    start = _free()                                                                  # with the three still alive: no cached room below
    plans, errors = [None] * 4, []
    gate = threading.Barrier(4)

    def create(i):
        try:
            torch.cuda.set_device(0)
            gate.wait()
            plans[i] = _plan(w, precision, schedule)
        except Exception as e:                                                      # noqa: BLE001 (reported below)
            errors.append(e)

    threads = [threading.Thread(target=create, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    try:
        assert not errors, errors
        four_cost = start - _free()
        print(f'{precision}-{schedule}: four plans from four threads cost {four_cost} bytes, one private plan {private_cost}; packed weights >= {pk}')
        for plan in plans:
            assert _same(_run(plan, frames[0]), ref)
        assert four_cost < 4 * private_cost - 3 * pk / 2, (four_cost, private_cost, pk)   # one copy of the weights, not four
    finally:
        for plan in plans:
            if plan is not None:
                plan.close()
    left = start - _free()                                                           # the four plans and the entry are gone
    for plan in held:
        plan.close()
    print(f'{precision}-{schedule}: {left} bytes not returned after every plan was closed')
    assert abs(left) <= GRANULE, left
