"""Both inference plans on the networks of tests/plan_zoo.py: graphs, paddings, sizes and channel counts the four reference models never
produce.  The criteria are the existing ones, unchanged (tests/layerwise.py): f16x2 - every stored tensor read back, error / E <= 1 for
every element against oracle/x2_bound.py's float64 chain from the GPU's own inputs, format health, as many tensors checked as the launch
list says are stored; f16 - tests/test_gpu_layers.py's 1-ulp criterion.  Then: the launch lists contain what the zoo is for, an image's
outputs do not depend on its batch mates, and the builder's refusals carry their texts.

A capped leaky activation is not among the refusals: compile_plan derives the cap from the activation code, so no NetSpec expresses one.

Measured worst error / E per zoo plan (one MI355X, B = 3): residual 0.558 (the standalone Add; convs <= 0.12), pyramid 0.217 fused /
0.284 one launch per layer, channels 0.573 / 0.582 (x:add_20), odd 0.548 (x:add_32) in all three schedules; worst over-estimate 2^8.3
(pyramid).  The standalone Add's ratio is large because its bound is small: one fp32 rounding of the sum plus the split store.

Sensitivity, carried out once and not committed: with xadd_kernel scaling its second operand by the FIRST operand's exponent, every spec
with a standalone Add fails in both f16x2 tests at that launch - x:add_16 error / E = 2.5e7, x:add_20 6.3e6, x:add_32 5.9e7 - and pyramid,
which has none, passes.  test_standalone_add_operands_have_different_exponents keeps that so: the operands' exponents differ by 2 or more
for every image (residual -8 / -10, channels -9..-8 / -7 and -10 / -7, odd -5..-6 / -8).

The cluster zoo (zoo.CLUSTER_ZOO; the test_cluster_* functions below): the latency schedule's x:persist[...] and x:heads[...] on the
instantiations yolo_mobilev1 0.75 at 224x320 leaves out, same criterion, no new tolerance.  zoo.persist_plan / zoo.heads_plan restate
the builders' choice of a variant and can drift there; block count, start shape, phase count, barrier count and the heads' phase list
are asserted against the launch names the builder emits.  Measured (one MI355X, B = 3), worst error / E per latency plan: cluster_wide
0.076, cluster_ragged 0.085, cluster_ring 0.079, cluster_deep 0.088 (each on a plain conv launch); worst x:persist store 0.036, worst
x:heads phase 0.042; throughput plans 0.133 / 0.131 / 0.150 / 0.118.  A store phase checked across TWO blocks sits at 0.002: that bound
is too wide to see a lost cross product, which is why every block of a chain is stored (plan_zoo._chain).
Sensitivity, carried out once and not committed, arithmetic only: (1) xp_pw_resident_loop without its w_hi * x_lo products where
NSH == 2 (adirect 3, resident - cluster_ring's pw_2 alone): that store fails with error / E = 21.2 (0.89, passing, while the bound
spanned two blocks); (2) xh_fill dropping the last K chunk where a phase has fewer chunks than the 8 members: all four specs fail at
x:heads, error / E = 9.4e4 (wide, pre_mid), 1.4e5 (ragged, up_mid), 3.5e3 (ring, head_mid + head_out), 7.9e4 (deep, up_only).  Under
either mutation tests/test_gpu_layers_x2.py::test_yolo_mobilev1_benched_network[latency-*] passes."""
import re
import time

import numpy as np
import pytest

from k210_yolo_framework_amd import netspec as ns
from tests import plan_zoo as zoo
from tests.layerwise import _frames, _layerwise, _layerwise_f16, _report, _switches
from tests.plan_zoo import Graph

pytestmark = pytest.mark.gpu

B = 3
UNFUSED = {'YK_FUSE_DWPW': '0', 'YK_SPLITK': '0', 'YK_FUSE_HEAD': '0'}
_specs = {}


def _spec(name):
    if name not in _specs:
        _specs[name] = (zoo.ZOO.get(name) or zoo.CLUSTER_ZOO[name])()
    return _specs[name]


def _count(names, pat):
    return sum(bool(re.search(pat, n)) for n in names)


def _launching_ops(spec):
    """ops that are a launch of their own when nothing is fused except the Adds yk_graph_analyse folds: every conv, depthwise conv and
    pool, and the Adds that are not folded"""
    g = Graph(spec)
    return sum(1 for i, op in enumerate(spec.ops)
               if op['type'] not in (ns.OP_UPSAMPLE, ns.OP_CONCAT) and not (op['type'] == ns.OP_ADD and g.folded_add(i) is not None))


# what each spec's throughput launch list must contain: (regular expression, number of launches it matches)
EXPECT = {
    'residual': [
        (r'^x:add_16$', 1),                                            # the Add of two Adds
        (r'\+add', 3),                                                 # swapped, usual, behind the biased conv
        (r'^x:stem3x3s2_16$', 1),                                      # a stem in front of a 1x1 conv: plain
        (r'^x:dw3x3s2_16\[', 1),                                       # 96 output pixels: not fused
        (r'\+upcat', 1),
    ],
    'pyramid': [
        (r'^x:add_', 0), (r'\+add', 2),
        (r'\+up\[', 2),                                                # 1x1 and 3x3 on upsample(a) alone
        (r'^x:conv1x1s1_64to32\+up\[', 1), (r'^x:conv3x3s1_64to12\+up\[', 1),
        (r'^x:conv1x1s1_84to36\+upcat\[', 1),                          # concat(upsample(a), b)
        (r'^x:conv3x3s1_68to192\+upcat\[', 1),                         # concat of two stored tensors; 192 -> 85 stays two launches
        (r'^x:conv1x1s1_192to85\[', 1),
        (r'^x:conv3x3s1_64to128\+conv1x1_128to80\[', 1),               # the widest output conv the fused head takes
        (r'^x:conv3x3s1_36to128\[', 1), (r'^x:conv1x1s1_128to18\[', 1),    # the middle tensor has a second reader
        (r'^x:stem3x3s2_24\+dw3x3s2\+conv1x1_24to20\[', 1),            # stride-2 stem + stride-2 depthwise, all padded (0, 1, 0, 1)
        (r'^x:dw3x3s2_36\[', 1), (r'^x:dw3x3s2_32\[', 1), (r'^x:dw3x3s2_8\[', 1),     # 117 output pixels < min_px = 128
        (r'dw3x3s2\+conv1x1_(36|32|8)to16', 0),
        (r'^x:conv3x3s2_20to64\[', 1),
        (r'^x:maxpool2x2s2_64$', 1),
    ],
    'channels': [
        (r'^x:stem3x3s1_32\+dw3x3s1\+conv1x1_32to12\[', 1),
        (r'^x:add_20$', 2), (r'\+add', 0),
        (r'^x:conv1x1s1_12to20\[', 1), (r'^x:conv3x3s1_12to36\[', 1), (r'^x:conv3x3s1_20to100\[', 1), (r'^x:conv1x1s1_36to20\[', 1),
        (r'^x:conv1x1s1_100to12\[', 1), (r'^x:conv1x1s1_20to18\[', 1),
        (r'^x:maxpool2x2s2_(12|20|36|100)$', 4), (r'^x:maxpool2x2s1_20$', 1),
    ],
    'odd': [
        (r'^x:stem3x3s2_16$', 1),                                      # in front of a 3x3 conv: plain
        (r'^x:dw3x3s2\+conv1x1_24to32\+add\[', 1),
        (r'^x:add_32$', 1),                                            # two convs between c1x1_p2 and its Add
        (r'^x:conv3x3s2_24to32\[', 1),
        (r'^x:maxpool2x2s2_24$', 2), (r'^x:maxpool2x2s1_24$', 1),
        (r'^x:conv3x3s1_32to128\+conv1x1_128to18\[', 1),
    ],
}


@pytest.mark.parametrize('name', list(zoo.ZOO))
def test_f16x2_every_launch_within_its_bound(name):
    t0 = time.time()
    spec, w = _spec(name)
    names, rows, over = _layerwise(spec, w, B)
    _report(f'zoo {name} {spec.in_hw[0]}x{spec.in_hw[1]} B={B} throughput', names, rows, over, t0)
    for pat, n in EXPECT[name]:
        assert _count(names, pat) == n, (pat, n, names)


@pytest.mark.parametrize('name', list(zoo.ZOO))
def test_f16x2_one_launch_per_layer(name):
    t0 = time.time()
    spec, w = _spec(name)
    names, rows, over = _layerwise(spec, w, B, env=UNFUSED)
    _report(f'zoo {name} B={B} unfused', names, rows, over, t0)
    assert len(rows) == _launching_ops(spec)
    assert not any('splitk' in n or '+dw3x3' in n or '+conv1x1_' in n for n in names), names


def test_f16x2_latency_schedule():
    """The latency schedule on `odd`.  By the builder's rules (x_read_opts, x_build_persist, x_build_heads): the heads launch switches the
    fused heads off, so head_mid and head_out are two launches; the persistent stage needs two depthwise + pointwise pairs of plain
    launches at multiples of 64 channels, which the spec does not have; the heads launch takes the plan's trailing run of conv launches
    when it has at least two, and here the run is out_2 alone (a standalone Add is in front of it).  Everything else is as in the
    throughput plan."""
    t0 = time.time()
    spec, w = _spec('odd')
    names, rows, over = _layerwise(spec, w, B, 'latency')
    _report(f'zoo odd B={B} latency', names, rows, over, t0)
    thr, _, _ = _layerwise(spec, w, B)
    assert not any(n.startswith(('x:persist', 'x:heads')) for n in names)
    assert _count(names, r'^x:conv3x3s1_32to128\[') == 1 and _count(names, r'^x:conv1x1s1_128to18\[') == 1
    fused = [n for n in thr if '+conv1x1_128to18' in n]
    assert [n for n in names if n in thr] == [n for n in thr if n not in fused] and len(names) == len(thr) + 1


def _standalone_adds(spec):
    g = Graph(spec)
    return [op for i, op in enumerate(spec.ops) if op['type'] == ns.OP_ADD and g.folded_add(i) is None]


@pytest.mark.parametrize('name', list(zoo.ZOO))
@pytest.mark.parametrize('fuse', [True, False])
def test_f16_every_launch(name, fuse):
    spec, w = _spec(name)
    n, names = _layerwise_f16(spec, w, B, fuse, fuse)
    print(f'\nzoo {name} f16 fuse={fuse}: {n} tensors checked; {names}')
    # every launch but u8_max leaves one tensor; a K-split conv leaves its tensor through its reduce launch, and a reduce launch that
    # ends in the 1x1 output conv leaves both
    assert n == len(names) - 1 - _count(names, r'/splitk\d+$') + _count(names, r'^splitk_reduce\d+_\d+\+conv')
    if not fuse:
        assert n == _launching_ops(spec)
    standalone = len(_standalone_adds(spec))
    assert _count(names, r'^add_') == standalone and _count(names, r'\+add') == sum(op['type'] == ns.OP_ADD for op in spec.ops) - standalone


@pytest.mark.parametrize('name', list(zoo.ZOO))
@pytest.mark.parametrize('env', [None, UNFUSED], ids=['default', 'unfused'])
def test_f16x2_an_image_does_not_depend_on_its_batch(name, env):
    """Bitwise: image 0 alone against image 0 of the batch, and the batch twice.  The default plan is the one that matters (fused blocks,
    fused heads whose K slices the last workgroup to arrive adds up, split-K); the switches are set here, not inherited from whatever ran before."""
    import torch
    from k210_yolo_framework_amd import engine
    spec, w = _spec(name)
    frames = torch.from_numpy(_frames(spec, B, seed=5)).cuda()
    with _switches(env), engine.Plan(spec, w, max_batch=B, precision='f16x2', schedule='throughput') as plan:
        names = [l[0] for l in plan.launches()]
        assert any('+conv1x1_' in n for n in names) == (env is None and name != 'residual'), names     # fused where the default plan fuses

        def run(f):
            plan.run_u8(f)
            plan.check()
            return [o[:f.shape[0]].cpu().numpy().copy() for o in plan.outputs()]
        first, second = run(frames), run(frames)
        alone = run(frames[:1].contiguous())
    for a, b, c in zip(first, second, alone):
        assert np.isfinite(a).all() and float(np.abs(a).max()) > 0
        assert a.tobytes() == b.tobytes(), 'two runs of the same batch differ'
        assert a[:1].tobytes() == c.tobytes(), 'image 0 alone differs from image 0 in the batch'


@pytest.mark.parametrize('name', [n for n in zoo.ZOO if n != 'pyramid'])
def test_standalone_add_operands_have_different_exponents(name):
    """What makes the layerwise check sensitive to xadd_kernel's rescaling: on the frames _layerwise uses, the two operands of every
    standalone Add are stored at different exponents for at least one image, so an Add that took one operand's exponent for both, or
    swapped them, would be wrong by a factor of two or more there - against a bound of 2^-22 of the sum."""
    import torch
    from k210_yolo_framework_amd import engine
    spec, w = _spec(name)
    adds = _standalone_adds(spec)
    assert adds
    with _switches(), engine.Plan(spec, w, max_batch=B, precision='f16x2', schedule='throughput') as plan:
        plan.run_u8(torch.from_numpy(_frames(spec, B, seed=0)).cuda())
        plan.check()
        for op in adds:
            e0, e1 = plan.read_exponents(op['in0'], B), plan.read_exponents(op['in1'], B)
            print(f'\nzoo {name} x:add_{op["cout"]} tensor {op["out"]}: operand exponents {e0.tolist()} and {e1.tolist()}')
            assert (e0 != e1).any(), (op, e0.tolist(), e1.tolist())


# what the f16 plan does with the graphs the f16x2 plan refuses: True = builds (and then passes its layerwise check), False = refuses
F16_BUILDS = {'refuse_residual_zoo_spec': True, 'refuse_concat24': True,          # its concat loader has no multiple-of-32 rule
              'refuse_stem20': False,                                           # 'stem conv Cout must be a multiple of 8'
              'refuse_concat_up_second': False, 'refuse_dw_on_upsample': False, 'refuse_dw_on_frame': False,
              'refuse_add_on_upsample': False, 'refuse_pool_on_view': False, 'refuse_output_not_flagged': False}


@pytest.mark.parametrize('case', zoo.REFUSALS, ids=[f.__name__ for f, _ in zoo.REFUSALS])
def test_refusals_by_name(case):
    import torch
    from k210_yolo_framework_amd import engine
    build, text = case
    spec, w = build()
    with _switches():
        with pytest.raises(engine.YkError, match=re.escape(text)):
            engine.Plan(spec, w, max_batch=B, precision='f16x2', schedule='throughput')
        try:
            engine.Plan(spec, w, max_batch=B, precision='f16').close()
            builds = True
        except engine.YkError as e:
            builds = False
            assert re.search(r'\): \S', str(e)), f'empty yk_last_error: {e}'
    print(f'\n{build.__name__}: f16 builds = {builds}')
    assert builds == F16_BUILDS[build.__name__]
    if builds:
        _layerwise_f16(spec, w, B)
    # a good plan still builds and runs in this process
    spec, w = _spec('channels')
    with _switches(), engine.Plan(spec, w, max_batch=B, precision='f16x2', schedule='throughput') as plan:
        assert any('+dw3x3' in l[0] for l in plan.launches())            # the default plan, whatever ran before
        plan.run_u8(torch.from_numpy(_frames(spec, B, seed=6)).cuda())
        plan.check()
        assert all(np.isfinite(o.cpu().numpy()).all() for o in plan.outputs())


# ---- the latency schedule's two cluster launches on the specs of zoo.CLUSTER_ZOO ----------------------------------------------------
NAME_MAX = 127                                                         # plan.launches() cuts a name there


def _cluster_names(spec):
    return zoo.persist_plan(spec)['name'][:NAME_MAX], zoo.heads_plan(spec)['name'][:NAME_MAX]


def _assert_cluster_launches(spec, names):
    """the builder took the chain and the convs the restatement says: block count, start shape, phase and barrier count, the heads' phase list"""
    persist, heads = _cluster_names(spec)
    assert [n for n in names if n.startswith('x:persist')] == [persist], names
    assert [n for n in names if n.startswith('x:heads')] == [heads], names
    assert names[-1] == heads


@pytest.mark.parametrize('name', list(zoo.CLUSTER_ZOO))
def test_cluster_launches_within_their_bound(name):
    """Latency schedule, the strict criterion of tests/layerwise.py, then the same plan with YK_CLUSTER_WT=1: every output bit for bit."""
    t0 = time.time()
    spec, w = _spec(name)
    names, rows, over = _layerwise(spec, w, B, 'latency')
    _report(f'zoo {name} {spec.in_hw[0]}x{spec.in_hw[1]} B={B} latency', names, rows, over, t0)
    _assert_cluster_launches(spec, names)
    t0 = time.time()
    names_wt, rows_wt, over = _layerwise(spec, w, B, 'latency', env={'YK_CLUSTER_WT': '1'})
    _report(f'zoo {name} B={B} latency YK_CLUSTER_WT=1', names_wt, rows_wt, over, t0)
    assert names_wt == names


@pytest.mark.parametrize('name', list(zoo.CLUSTER_ZOO))
def test_cluster_specs_as_plain_launches(name):
    """The same shapes in the throughput schedule (fused blocks up to 384 input channels, fused heads, K-split convs) and in the f16 plan."""
    t0 = time.time()
    spec, w = _spec(name)
    names, rows, over = _layerwise(spec, w, B)
    _report(f'zoo {name} B={B} throughput', names, rows, over, t0)
    assert not any(n.startswith(('x:persist', 'x:heads')) for n in names)
    n, names = _layerwise_f16(spec, w, B)
    print(f'\nzoo {name} f16: {n} tensors checked; {names}')
    assert n == len(names) - 1 - _count(names, r'/splitk\d+$') + _count(names, r'^splitk_reduce\d+_\d+\+conv')


@pytest.mark.parametrize('name', list(zoo.CLUSTER_ZOO))
def test_cluster_launches_do_not_depend_on_the_batch(name):
    """Bitwise: the batch twice, the same plan with YK_CLUSTER_WT=1, image 0 alone in a plan for two, and images 0..2 of a batch of 40 (more
    images than one pass of the 32 clusters).  plan.check() behind every run: a cluster that cannot assemble is an error, not a wait."""
    import torch
    from k210_yolo_framework_amd import engine
    spec, w = _spec(name)
    frames = _frames(spec, B, seed=5)
    big = np.concatenate([frames, np.random.default_rng(6).integers(0, 256, (40 - B, *frames.shape[1:]), dtype=np.uint8)])

    def run(f, max_batch, env=None):
        f = torch.from_numpy(np.ascontiguousarray(f)).cuda()
        with _switches(env), engine.Plan(spec, w, max_batch=max_batch, precision='f16x2', schedule='latency') as plan:
            _assert_cluster_launches(spec, [l[0] for l in plan.launches()])
            outs = []
            for _ in range(2):
                plan.run_u8(f)
                plan.check()
                outs.append([o[:f.shape[0]].cpu().numpy().copy() for o in plan.outputs()])
        for a, b in zip(*outs):
            assert np.isfinite(a).all() and float(np.abs(a).max()) > 0
            assert a.tobytes() == b.tobytes(), 'two runs of the same batch differ'
        return outs[0]
    first = run(frames, B)
    for what, other in (('YK_CLUSTER_WT=1', run(frames, B, {'YK_CLUSTER_WT': '1'})), ('image 0 alone', run(frames[:1], 2)),
                        ('a batch of 40', run(big, 40))):
        for a, b in zip(first, other):
            k = min(len(a), len(b), B)
            assert a[:k].tobytes() == b[:k].tobytes(), f'{what}: differs from the batch of {B}'
