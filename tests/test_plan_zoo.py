"""tests/plan_zoo.py on the CPU: (1) the two oracles the GPU tests trust - oracle/x2_bound.run_chain (torch float64) and the fp32 C
interpreter oracle.net_forward_ex - agree on every tensor of every zoo spec, to the tolerance tests/test_oracle_net.py holds fp32 against
float64 to (2e-5 of the tensor's maximum); (2) every feature the zoo's docstrings claim is found in spec.ops itself, so that an edit to
the zoo cannot drop one silently."""
import numpy as np
import pytest

import oracle
from k210_yolo_framework_amd import netspec as ns
from oracle import x2_bound as xb
from tests import plan_zoo as zoo
from tests.layerwise import _frames

CONVS = (ns.OP_CONV, ns.OP_DWCONV)
VIEWS = zoo.VIEWS


@pytest.mark.parametrize('name', list(zoo.ZOO))
def test_float64_chain_agrees_with_fp32_interpreter(name):
    spec, w = zoo.ZOO[name]()
    cp = spec.compile_plan(w)
    x32 = oracle.normalise_u8(_frames(spec, 3, seed=3))
    want = [op['out'] for op in spec.ops]
    got = oracle.net_forward_ex(cp, {0: x32}, range(len(spec.ops)), want, emulate_f16=False)
    ref, _ = xb.run_chain(spec, w, {0: x32.astype(np.float64)}, bounds=False)
    for t, g in zip(want, got):
        r = ref[t]
        assert g.shape == r.shape == (3, *spec.tensors[t])
        scale = max(float(np.abs(r).max()), 1e-6)
        assert float(np.abs(g - r).max()) / scale < 2e-5, (t, float(np.abs(g - r).max()), scale)
    for t in spec.outputs:
        assert float(np.abs(ref[t]).max()) > 1e-3                      # a dead network would agree with anything


# ---- what the specs contain, from spec.ops (zoo.Graph) --------------------------------------------------------------
@pytest.fixture(scope='module')
def graphs():
    return {n: zoo.Graph(f()[0]) for n, f in zoo.ZOO.items()}


def _any(graphs, pred):
    """names of the specs in which some op index satisfies pred(graph, index)"""
    return [n for n, g in graphs.items() if any(pred(g, i) for i in range(len(g.ops)))]


def test_the_zoo_contains_the_wiring_of_residual_zoo_spec(graphs):
    """the same ops up to the head; the head differs only in the width of the conv in front of the upsample (8 -> 32: the f16x2 concat
    takes its first source in multiples of 32 channels)"""
    from tests.mini_net import residual_zoo_spec
    mine, theirs = graphs['residual'].ops, residual_zoo_spec().ops
    assert len(mine) == len(theirs)
    for a, b in zip(mine, theirs):
        assert {k: v for k, v in a.items() if k not in ('cin', 'cout')} == {k: v for k, v in b.items() if k not in ('cin', 'cout')}
    assert sum(a != b for a, b in zip(mine, theirs)) == 4              # that conv, the upsample, the concat and the conv behind it


def test_item1_adds(graphs):
    def standalone(g, i):
        return g.ops[i]['type'] == ns.OP_ADD and g.folded_add(i) is None
    assert _any(graphs, lambda g, i: standalone(g, i) and g.kind(g.ops[i]['in0']) == ns.OP_ADD and g.kind(g.ops[i]['in1']) == ns.OP_ADD)
    # a conv operand with a second reader: the conv sits right in front of the Add and would fold but for uses == 2
    assert _any(graphs, lambda g, i: standalone(g, i) and g.ops[i - 1]['type'] == ns.OP_CONV and
                g.ops[i - 1]['out'] in (g.ops[i]['in0'], g.ops[i]['in1']) and g.uses[g.ops[i - 1]['out']] == 2)
    # not adjacent: an operand is a conv's output with one reader, but the op before the Add produces neither operand
    assert _any(graphs, lambda g, i: standalone(g, i) and g.ops[i - 1]['out'] not in (g.ops[i]['in0'], g.ops[i]['in1']) and
                any(g.kind(t) == ns.OP_CONV and g.uses[t] == 1 for t in (g.ops[i]['in0'], g.ops[i]['in1'])))
    assert _any(graphs, lambda g, i: standalone(g, i) and g.shape(g.ops[i]['out'])[2] % 8 != 0)
    assert _any(graphs, lambda g, i: g.folded_add(i) is not None and g.ops[i]['in0'] == g.ops[i - 1]['out'])      # conv output as in0
    assert _any(graphs, lambda g, i: g.folded_add(i) is not None and g.ops[i]['in1'] == g.ops[i - 1]['out'])      # the usual order
    assert _any(graphs, lambda g, i: g.folded_add(i) is not None and i >= 2 and g.dw_fused(i - 2))                # folded into a fused block


def test_item2_padding(graphs):
    same = (0, 1, 0, 1)

    def s2(g, i, ty):
        return g.ops[i]['type'] == ty and g.ops[i]['stride'] == 2 and g.pad(g.ops[i]) == same
    assert _any(graphs, lambda g, i: s2(g, i, ns.OP_CONV) and g.ops[i]['in0'] == 0)
    assert _any(graphs, lambda g, i: s2(g, i, ns.OP_DWCONV) and g.dw_fused(i))
    small = _any(graphs, lambda g, i: s2(g, i, ns.OP_DWCONV) and not g.dw_fused(i) and g.dw_fused(i, min_px=0) and
                 np.prod(g.shape(g.ops[i]['out'])[:2]) < 128)
    assert small                                                        # every other fusion condition holds: only min_px keeps it apart
    assert _any(graphs, lambda g, i: s2(g, i, ns.OP_CONV) and g.plain_conv(i) and g.ops[i]['k'] == 3)
    assert _any(graphs, lambda g, i: g.ops[i]['type'] == ns.OP_DWCONV and g.ops[i]['stride'] == 2 and g.pad(g.ops[i]) == (1, 0, 1, 0))
    for g in graphs.values():                                           # Keras 'same' means (0, 1) only on an even size
        for op in g.ops:
            if op['type'] in CONVS and g.pad(op) == same:
                assert g.shape(op['in0'])[0] % 2 == 0 and g.shape(op['in0'])[1] % 2 == 0


def test_item3_odd_sizes(graphs):
    g = graphs['odd']
    assert g.spec.in_hw[0] % 2 == 1 and g.spec.in_hw[1] % 2 == 1

    def on_odd(i):
        h, w_, _ = g.shape(g.ops[i]['in0'])
        return h % 2 == 1 and w_ % 2 == 1
    n = range(len(g.ops))
    assert any(g.ops[i]['type'] == ns.OP_CONV and g.ops[i]['in0'] == 0 and g.ops[i]['stride'] == 2 for i in n)
    assert any(g.ops[i]['type'] == ns.OP_MAXPOOL and g.ops[i]['stride'] == 2 and on_odd(i) for i in n)
    assert any(g.ops[i]['type'] == ns.OP_MAXPOOL and g.ops[i]['stride'] == 1 for i in n)
    assert any(g.ops[i]['type'] == ns.OP_DWCONV and g.ops[i]['stride'] == 2 and on_odd(i) for i in n)
    assert any(g.ops[i]['type'] == ns.OP_CONV and g.ops[i]['k'] == 3 and g.ops[i]['stride'] == 2 and g.plain_conv(i) and on_odd(i) for i in n)
    # a head on an odd level of the even pyramid, upsampled to exactly the size of its concat partner
    p = graphs['pyramid']
    assert any(p.shape(t)[0] % 2 == 1 and p.shape(t)[1] % 2 == 1 for t in p.spec.outputs)


def test_item4_views(graphs):
    def reads(g, i, k):
        return g.ops[i]['type'] == ns.OP_CONV and g.ops[i]['k'] == k

    def cat(g, i):
        c = g.prod(g.ops[i]['in0'])
        return c if c and c['type'] == ns.OP_CONCAT else None
    assert _any(graphs, lambda g, i: reads(g, i, 1) and g.kind(g.ops[i]['in0']) == ns.OP_UPSAMPLE)
    assert _any(graphs, lambda g, i: reads(g, i, 3) and g.kind(g.ops[i]['in0']) == ns.OP_UPSAMPLE)
    assert _any(graphs, lambda g, i: reads(g, i, 3) and cat(g, i) and g.kind(cat(g, i)['in0']) not in VIEWS and
                g.kind(cat(g, i)['in1']) not in VIEWS)
    assert _any(graphs, lambda g, i: reads(g, i, 1) and cat(g, i) and g.kind(cat(g, i)['in0']) == ns.OP_UPSAMPLE and
                g.kind(cat(g, i)['in1']) not in VIEWS)
    for op in graphs['pyramid'].ops:                                   # a: cp % 32 == 0; b: a ragged last channel group
        if op['type'] == ns.OP_CONCAT:
            assert graphs['pyramid'].shape(op['in0'])[2] in (32, 64) and graphs['pyramid'].shape(op['in1'])[2] % 8 != 0


def test_item5_channels(graphs):
    for c in (12, 20, 36, 100):
        for what, pred in (('plain 1x1 conv', lambda g, i: g.plain_conv(i) and g.ops[i]['k'] == 1 and not g.ops[i]['flags']),
                           ('plain 3x3 conv', lambda g, i: g.plain_conv(i) and g.ops[i]['k'] == 3),
                           ('pool', lambda g, i: g.ops[i]['type'] == ns.OP_MAXPOOL)):
            hit = _any(graphs, lambda g, i: pred(g, i) and c in (g.shape(g.ops[i]['in0'])[2], g.shape(g.ops[i]['out'])[2]) and
                       g.kind(g.ops[i]['in0']) not in VIEWS)
            assert hit, f'no {what} on a stored {c}-channel tensor'


def test_item6_heads(graphs):
    def head(g, i, mid, out):
        return i + 1 < len(g.ops) and g.ops[i]['type'] == ns.OP_CONV and g.ops[i]['k'] == 3 and g.ops[i]['cout'] == mid and \
            g.ops[i + 1]['in0'] == g.ops[i]['out'] and g.ops[i + 1]['cout'] == out and (g.ops[i + 1]['flags'] & ns.FLAG_NET_OUTPUT)
    assert _any(graphs, lambda g, i: head(g, i, 128, 80) and g.head_fuses(i))
    assert _any(graphs, lambda g, i: head(g, i, 192, 85) and not g.head_fuses(i) and g.uses[g.ops[i]['out']] == 1)       # only the width is in the way
    assert _any(graphs, lambda g, i: g.ops[i]['cout'] == 128 and i + 1 < len(g.ops) and head(g, i, 128, g.ops[i + 1]['cout']) and
                g.ops[i + 1]['cout'] <= 80 and g.uses[g.ops[i]['out']] == 2 and not g.head_fuses(i))
    assert _any(graphs, lambda g, i: g.ops[i]['cout'] == 18 and (g.ops[i]['flags'] & ns.FLAG_NET_OUTPUT))
    s = graphs['pyramid'].spec
    assert s.anchor_num * (5 + s.class_num) == 80


def test_item7_stems(graphs):
    stems = {n: g.ops[0] for n, g in graphs.items()}
    assert all(o['type'] == ns.OP_CONV and o['in0'] == 0 and o['k'] == 3 for o in stems.values())
    assert {o['cout'] for o in stems.values()} == {16, 24, 32}

    def stem_fused(g):                                                 # decide_stem: the stem's only reader is the depthwise conv of a fused block
        return g.ops[1]['type'] == ns.OP_DWCONV and g.ops[1]['in0'] == g.ops[0]['out'] and g.uses[g.ops[0]['out']] == 1 and \
            g.dw_fused(1, min_px=128) and g.ops[2]['cout'] <= 64 and g.ops[0]['cout'] <= 32
    assert any(stem_fused(g) and g.ops[0]['stride'] == 1 for g in graphs.values())
    assert any(stem_fused(g) and g.ops[0]['stride'] == 2 and g.ops[1]['stride'] == 2 for g in graphs.values())
    assert any(g.ops[1]['type'] == ns.OP_CONV and g.ops[1]['k'] == 3 and g.ops[1]['in0'] == g.ops[0]['out'] for g in graphs.values())


def test_item8_activations(graphs):
    def act(g, i, ty, a):
        return g.ops[i]['type'] == ty and (g.ops[i]['act'], g.ops[i]['alpha']) == a
    assert _any(graphs, lambda g, i: act(g, i, ns.OP_DWCONV, ns.LEAKY01))
    assert _any(graphs, lambda g, i: act(g, i, ns.OP_DWCONV, (ns.ACT_NONE, 0.0)))
    assert _any(graphs, lambda g, i: act(g, i, ns.OP_CONV, ns.RELU) and g.ops[i]['k'] == 1)
    assert _any(graphs, lambda g, i: act(g, i, ns.OP_CONV, ns.RELU6) and g.ops[i]['k'] == 3 and g.ops[i]['in0'] != 0)


def test_a_tensor_read_only_by_a_depthwise_launch(graphs):
    """the fp32-plane store of a plain conv (xg_epilogue's dst_f32) feeding a depthwise launch of its own"""
    assert _any(graphs, lambda g, i: g.ops[i]['type'] == ns.OP_DWCONV and not g.dw_fused(i) and g.uses[g.ops[i]['in0']] == 1 and
                g.kind(g.ops[i]['in0']) == ns.OP_CONV and g.plain_conv(g.producer[g.ops[i]['in0']]) and
                g.folded_add(g.producer[g.ops[i]['in0']] + 1) is None)


def test_refusal_graphs_are_well_formed_for_the_oracle():
    """Each refused graph is still a computable network (the refusal is the plan's, not the graph's): the float64 chain runs it."""
    for f, text in zoo.REFUSALS:
        spec, w = f()
        assert text
        x = oracle.normalise_u8(_frames(spec, 1, seed=1)).astype(np.float64)
        ref, _ = xb.run_chain(spec, w, {0: x}, bounds=False)
        assert all(np.isfinite(ref[t]).all() for t in spec.outputs)


# ---- the cluster zoo: which instantiations of x:persist / x:heads each spec reaches (zoo.persist_plan, zoo.heads_plan) ----------------
# persist: (nrb, ncb, adirect, resident, ppw, WR, WC) per block, worked out by hand from x_build_persist; stores: an XP_STORE behind the
# block; heads: (variant, nrb, ncb, nchunk, tail, pre_barrier) per phase in the launch's order, from x_build_heads_from
CLUSTER_EXPECT = {
    'cluster_wide': dict(
        src_f32=True,
        persist=[(20, 1, 0, 0, 6, 8, 1), (5, 1, 2, 0, 3, 8, 1), (5, 5, 2, 0, 3, 4, 2), (5, 2, 2, 0, 3, 8, 1), (5, 8, 2, 0, 4, 2, 4)],
        stores=[1, 1, 1, 1, 1],
        heads=[(2, 5, 4, 4, 0, 0), (2, 5, 1, 2, 0, 1), (1, 5, 12, 4, 75, 0)]),
    'cluster_ragged': dict(
        src_f32=False,
        persist=[(9, 3, 1, 1, 3, 8, 1), (9, 4, 0, 0, 4, 4, 2), (9, 3, 1, 0, 3, 8, 1), (3, 5, 0, 0, 3, 4, 2), (3, 2, 3, 0, 3, 4, 2),
                 (3, 8, 0, 0, 3, 1, 8)],
        stores=[1, 1, 1, 1, 1, 1],
        heads=[(2, 3, 4, 4, 0, 0), (1, 3, 3, 4, 18, 0), (1, 3, 5, 4, 0, 0), (0, 9, 8, 10, 80, 0)]),
    'cluster_ring': dict(
        src_f32=True,
        persist=[(6, 1, 0, 0, 3, 8, 1), (6, 2, 3, 1, 3, 8, 1), (6, 12, 0, 0, 5, 2, 4)],
        stores=[1, 1, 1],
        heads=[(0, 6, 8, 4, 18, 1)]),
    'cluster_deep': dict(
        src_f32=True,
        persist=[(5, 3, 2, 0, 3, 8, 1), (5, 1, 2, 0, 3, 8, 1), (5, 10, 4, 0, 4, 2, 4)],
        stores=[1, 1, 1],
        heads=[(2, 5, 2, 4, 0, 0), (2, 5, 4, 4, 18, 0), (1, 5, 8, 4, 18, 0)]),
}


@pytest.fixture(scope='module')
def cluster_specs():
    return {n: f() for n, f in zoo.CLUSTER_ZOO.items()}


@pytest.mark.parametrize('name', list(zoo.CLUSTER_ZOO))
def test_cluster_spec_reaches_the_expected_instantiations(cluster_specs, name):
    spec, _ = cluster_specs[name]
    want = CLUSTER_EXPECT[name]
    p, h = zoo.persist_plan(spec), zoo.heads_plan(spec)
    assert p and h
    assert [tuple(b[k] for k in ('nrb', 'ncb', 'adirect', 'resident', 'ppw', 'WR', 'WC')) for b in p['blocks']] == want['persist']
    assert [int(b['store']) for b in p['blocks']] == want['stores'] and p['src_f32'] == want['src_f32']
    assert [tuple(q[k] for k in ('variant', 'nrb', 'ncb', 'nchunk', 'tail', 'pre_barrier')) for q in h['phases']] == want['heads']
    # the chain is made of launches the latency schedule keeps apart: fewer than 128 output pixels, or more than 6 steps of 32 channels
    for b in p['blocks']:
        assert b['H'] * b['W'] < 128 or b['cin'] >= 224
        assert b['cin'] % 64 == 0 and b['n'] % 128 == 0 and b['nrb'] + b['ncb'] <= 24
    assert spec.in_hw[0] <= 64 and spec.in_hw[1] <= 96


def test_cluster_zoo_covers_every_target(cluster_specs):
    hit = {n: zoo.cluster_targets(s) for n, (s, _) in cluster_specs.items()}
    union = set().union(*hit.values())
    for t in sorted(zoo.CLUSTER_TARGETS):
        print(f'{t:60s} {[n for n in hit if t in hit[n]]}')
    assert zoo.CLUSTER_TARGETS <= union, sorted(zoo.CLUSTER_TARGETS - union)
    # both kinds of chain input, and a heads phase that reads what the persistent launch stored in mid-chain
    assert 'chain from fp32 planes' in union and 'chain from a split tensor' in union
    spec, _ = cluster_specs['cluster_wide']
    p, h = zoo.persist_plan(spec), zoo.heads_plan(spec)
    mid = {spec.ops[b['op'] + 1]['out'] for b in p['blocks'][:-1] if b['store']}
    assert any(set(q['srcs']) & mid for q in h['phases'])


def test_the_benched_network_reaches_none_of_the_targets():
    """yolo_mobilev1 0.75 at 224x320 is the one network tests/test_gpu_layers_x2.py holds to the strict criterion in the latency schedule;
    the restatement reproduces its two launch names (tests/golden/x2_plan_launches.json), and none of the targets is among what it reaches."""
    import json
    from pathlib import Path
    spec = ns.yolo_mobilev1((224, 320, 3), 3, 20, alpha=0.75)
    p, h = zoo.persist_plan(spec), zoo.heads_plan(spec)
    golden = json.dumps(json.loads((Path(__file__).parent / 'golden' / 'x2_plan_launches.json').read_text()))
    assert json.dumps(p['name'])[1:-1] in golden and json.dumps(h['name'][:127])[1:-1] in golden
    assert [(b['nrb'], b['ncb'], b['adirect'], b['resident']) for b in p['blocks']] == [(18, 3, 1, 1)] * 5 + [(5, 6, 2, 0)] * 2
    assert [(q['variant'], q['nrb'], q['nchunk']) for q in h['phases']] == [(2, 5, 24), (1, 5, 24), (0, 18, 16)]
    assert not zoo.cluster_targets(spec) & zoo.CLUSTER_TARGETS


@pytest.mark.parametrize('name', list(zoo.CLUSTER_ZOO))
def test_float64_chain_agrees_with_fp32_interpreter_on_the_cluster_zoo(cluster_specs, name):
    spec, w = cluster_specs[name]
    cp = spec.compile_plan(w)
    x32 = oracle.normalise_u8(_frames(spec, 3, seed=3))
    want = [op['out'] for op in spec.ops]
    got = oracle.net_forward_ex(cp, {0: x32}, range(len(spec.ops)), want, emulate_f16=False)
    ref, _ = xb.run_chain(spec, w, {0: x32.astype(np.float64)}, bounds=False)
    for t, g in zip(want, got):
        r = ref[t]
        scale = max(float(np.abs(r).max()), 1e-6)
        assert g.shape == r.shape and float(np.abs(g - r).max()) / scale < 2e-5, (t, float(np.abs(g - r).max()), scale)
    for t in spec.outputs:
        assert float(np.abs(ref[t]).max()) > 1e-3
