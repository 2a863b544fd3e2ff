"""Small networks the four reference models never produce, for the inference plans (tests/test_plan_zoo.py checks on the CPU that every
feature named here is really in spec.ops; tests/test_gpu_plan_zoo.py runs them through both plans).  NetSpec is a general builder and
yk_plan_create takes any op table: every function returns (NetSpec, weights).  The item numbers in the docstrings:

  1 Adds       standalone (an Add of two Adds, an Add whose conv operand has a second reader, an Add not adjacent to its conv, one on a
               tensor with c % 8 != 0) and folded (conv output as in0, and the usual order)
  2 padding    stride 2 with pad (0, 1, 0, 1) - Keras 'same' on an even size - on the stem, a fused depthwise conv, a depthwise conv that
               stays a launch of its own (< 128 output pixels) and a 3x3 conv; a depthwise conv with (1, 0, 1, 0)
  3 odd sizes  an odd input; stride-2 pool on odd h and w, a stride-1 pool, a stride-2 depthwise and a stride-2 3x3 conv on odd sizes
  4 views      1x1 and 3x3 conv on upsample(a) alone, 3x3 conv on concat(a, b) of two real tensors, 1x1 conv on concat(upsample(a), b)
  5 channels   stored tensors of 12, 20, 36 and 100 channels, each read or written by a plain 1x1 conv, a plain 3x3 conv and a pool
  6 heads      128 -> 80 (fuses), 192 -> 85 (too wide), 128 with a second reader of the middle tensor (must not fuse), an 18-channel output
  7 stems      16 / 24 / 32 filters; stride 1 in front of a depthwise conv, stride 2 in front of a stride-2 depthwise conv, a stem in
               front of a 3x3 conv
  8 activations  depthwise + LeakyReLU(0.1), depthwise without activation, pointwise + ReLU, 3x3 + ReLU6"""
from k210_yolo_framework_amd import netspec as ns
from tests.mini_net import residual_zoo_spec

NONE = (ns.ACT_NONE, 0.0)
KERAS_SAME_S2 = (0, 1, 0, 1)            # (top, bottom, left, right): what Keras 'same' pads at stride 2 on an even size
DARKNET_S2 = (1, 0, 1, 0)

VIEWS = (ns.OP_UPSAMPLE, ns.OP_CONCAT)


class Graph:
    """Use counts, producers and the plan builders' fold / fuse rules (yk_graph_analyse, decide_blocks, decide_fin_heads of
    csrc/yk_plan_graph.h and yk_xplan_build.h) restated over spec.ops, for the tests to say what a spec contains.  A copy can drift: the
    launch-name assertions of tests/test_gpu_plan_zoo.py hold it against what the builder really emits."""
    def __init__(self, spec):
        self.spec, self.ops = spec, spec.ops
        self.producer = {op['out']: i for i, op in enumerate(spec.ops)}
        self.uses = {}
        for op in spec.ops:
            for t in (op['in0'], op['in1']):
                if t >= 0:
                    self.uses[t] = self.uses.get(t, 0) + 1
        for t in spec.outputs:
            self.uses[t] = self.uses.get(t, 0) + 1

    def prod(self, t):
        return self.ops[self.producer[t]] if t in self.producer else None

    def kind(self, t):
        p = self.prod(t)
        return p['type'] if p else None

    def shape(self, t):
        return self.spec.tensors[t]

    def pad(self, op):
        return (op['pad_t'], op.get('pad_b'), op['pad_l'], op.get('pad_r'))

    def folded_add(self, i):
        """yk_graph_analyse's rule: the op before the Add is a conv that produces one operand, read by nothing else; the other operand
        is a stored tensor.  -> the conv's index or None."""
        q = self.ops[i]
        if q['type'] != ns.OP_ADD or i == 0:
            return None
        o = self.ops[i - 1]
        y = o['out']
        if o['type'] != ns.OP_CONV or (o['flags'] & ns.FLAG_NET_OUTPUT) or y not in (q['in0'], q['in1']) or q['in0'] == q['in1']:
            return None
        other = q['in1'] if q['in0'] == y else q['in0']
        if self.uses[y] != 1 or other == 0 or self.kind(other) in VIEWS:
            return None
        return i - 1

    def dw_fused(self, i, min_px=128):
        """decide_blocks: a depthwise conv on a stored tensor whose only reader is the next op, a 1x1 stride-1 conv; >= 128 output pixels."""
        o = self.ops[i]
        if o['type'] != ns.OP_DWCONV or i + 1 >= len(self.ops):
            return False
        q = self.ops[i + 1]
        h, w_, _ = self.shape(o['out'])
        return (q['type'] == ns.OP_CONV and q['k'] == 1 and q['stride'] == 1 and q['in0'] == o['out'] and self.uses[o['out']] == 1 and
                o['in0'] != 0 and self.kind(o['in0']) not in VIEWS and not (q['flags'] & ns.FLAG_NET_OUTPUT) and h * w_ >= min_px)

    def plain_conv(self, i):
        """a conv that is neither the stem nor the pointwise half of a fused block"""
        o = self.ops[i]
        return o['type'] == ns.OP_CONV and o['in0'] != 0 and not (i > 0 and self.dw_fused(i - 1))

    def head_fuses(self, i):
        """decide_fin_heads: a 128- / 192-wide stride-1 conv whose only reader is the next op, a 1x1 NET_OUTPUT conv of at most 80 channels."""
        o = self.ops[i]
        if not self.plain_conv(i) or o['cout'] not in (128, 192) or o['stride'] != 1 or i + 1 >= len(self.ops):
            return False
        q = self.ops[i + 1]
        return (q['type'] == ns.OP_CONV and bool(q['flags'] & ns.FLAG_NET_OUTPUT) and q['k'] == 1 and q['in0'] == o['out'] and
                q['cout'] <= 80 and self.uses[o['out']] == 1 and self.folded_add(i + 1) is None)


def residual():
    """The wiring of tests/mini_net.py::residual_zoo_spec, 32x48, with a head the f16x2 plan accepts (residual_zoo_spec itself upsamples
    8 channels into its concat and is on the refusal list below).  Item 1: Add(conv output, shortcut) folded with the operands swapped, a
    folded Add in the usual order, an Add of two Adds (standalone), a biased BatchNorm-free conv feeding a folded Add.  Item 7: a
    16-filter stride-2 stem in front of a 1x1 conv (a launch of its own).  Its stride-2 depthwise conv has 96 output pixels: not fused."""
    s = ns.NetSpec('zoo_residual', (32, 48), anchor_num=3, class_num=20)
    x = s._new_tensor(32, 48, 3)
    x = s.conv(x, 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='conv1')
    a = s.conv(x, 16, 1, act=ns.RELU6, name='conv_a')
    r1 = s.add(a, x)                                       # operands swapped: (conv output, shortcut)
    b = s.conv(r1, 16, 1, act=ns.LEAKY03, name='conv_b')
    r2 = s.add(r1, b)                                      # the usual order
    r3 = s.add(r2, r1)                                     # r2 and r1 are both Adds; r1 has three readers
    c = s.conv(r3, 16, 1, bn=False, bias=True, name='conv_c')
    r4 = s.add(r3, c)
    x1 = s.conv(r4, 16, 1, act=ns.LEAKY03, name='conv_pw_1')
    t = s.dwconv(x1, 2, ns.K210_S2_PAD, act=ns.RELU, name='conv_dw_2')
    x2 = s.conv(t, 32, 1, act=ns.LEAKY03, name='conv_pw_2')
    ns._head(s, x1, x2, 24, 16, 32, 75, [0])               # (residual_zoo_spec: 8 channels through the upsample)
    return s, s.init_weights(seed=11)


def pyramid():
    """72x104 -> 36x52 -> 18x26 -> 9x13 (odd) -> 5x7.
    Item 2: every strided layer pads (0, 1, 0, 1) - stem, dw_1 (fused with pw_1 and the stem), dw_small / dw_planes (117 output pixels:
    launches of their own), down_3x3; dw_dark pads (1, 0, 1, 0).  Item 3: a stride-2 pool on the odd 9x13 level.
    Item 4: up_1x1 and up_3x3 read upsample(a) alone, upcat_1x1 reads concat(upsample(a), b), head85_mid (3x3) reads concat(up_1x1, m) of
    two real tensors; a has 64 and up_1x1 32 channels, b 20 and m 36.  Item 5: 12, 20 and 36 channels on plain convs.
    Item 6: 128 -> 80 on the odd level, 192 -> 85, and shared_mid (128) -> 18 whose middle tensor shared_second_reader also reads.
    Item 7: 24 filters, stride 2, in front of a stride-2 depthwise conv.  Item 8: dw_1 LeakyReLU(0.1), dw_planes none, pw_1 ReLU.
    Item 1: two folded Adds behind plain 1x1 convs.  shared_second_reader's only reader is a depthwise launch: fp32 planes."""
    s = ns.NetSpec('zoo_pyramid', (72, 104), anchor_num=5, class_num=11)
    x = s._new_tensor(72, 104, 3)
    x = s.conv(x, 24, 3, 2, KERAS_SAME_S2, act=ns.LEAKY03, name='stem')                    # 36x52x24
    d = s.dwconv(x, 2, KERAS_SAME_S2, act=ns.LEAKY01, name='dw_1')                         # 18x26x24
    b = s.conv(d, 20, 1, act=ns.RELU, name='pw_1')                                         # 18x26x20
    a = s.conv(b, 64, 3, 2, KERAS_SAME_S2, act=ns.LEAKY01, name='down_3x3')                # 9x13x64
    t = s.conv(a, 128, 3, act=ns.LEAKY01, name='head80_mid')
    y1 = s.conv(t, 80, 1, bn=False, bias=True, name='head80_out', net_output=True)
    s.maxpool(a, 2)                                                                        # 5x7x64
    u = s.upsample(a)                                                                      # 18x26x64, a view
    u1 = s.conv(u, 32, 1, act=ns.LEAKY01, name='up_1x1')
    s.conv(u, 12, 3, act=ns.LEAKY03, name='up_3x3')
    m = s.conv(s.concat(u, b), 36, 1, act=ns.LEAKY01, name='upcat_1x1')                    # 18x26x36
    k = s.conv(s.concat(u1, m), 192, 3, act=ns.LEAKY01, name='head85_mid')
    y2 = s.conv(k, 85, 1, bn=False, bias=True, name='head85_out', net_output=True)
    h = s.conv(m, 128, 3, act=ns.LEAKY01, name='shared_mid')
    y3 = s.conv(h, 18, 1, bn=False, bias=True, name='shared_out', net_output=True)
    z = s.conv(h, 8, 1, act=ns.RELU, name='shared_second_reader')                          # 18x26x8
    e = s.conv(s.dwconv(m, 2, KERAS_SAME_S2, act=ns.RELU, name='dw_small'), 16, 1, act=ns.LEAKY03, name='pw_small')      # 9x13x16
    f = s.conv(s.dwconv(u1, 2, DARKNET_S2, act=ns.RELU6, name='dw_dark'), 16, 1, act=ns.LEAKY03, name='pw_dark')
    r = s.add(e, f)
    g = s.conv(s.dwconv(z, 2, KERAS_SAME_S2, act=NONE, name='dw_planes'), 16, 1, act=NONE, name='pw_planes')
    s.add(r, g)
    s.outputs = [y1, y2, y3]
    return s, s.init_weights(seed=12)


def channels():
    """24x32, every tensor at that size or half of it.
    Item 5: tensors of 12, 20, 36 and 100 channels; each is the input or output of a plain 1x1 conv, of a plain 3x3 conv, and the input of
    a pool.  Item 1: Add(t20, c1x1_36to20) where a stride-1 pool also reads the conv's output (uses = 2: standalone, 20 channels), then an
    Add of that Add and the pool.  Item 6: an 18-channel output.  Item 7: 32 filters, stride 1, fused with dw_1 + pw_1.
    Item 8: dw_1 without activation, c1x1_12to20 ReLU, c3x3_12to36 ReLU6."""
    s = ns.NetSpec('zoo_channels', (24, 32), anchor_num=3, class_num=1)
    x = s._new_tensor(24, 32, 3)
    x = s.conv(x, 32, 3, 1, None, act=ns.RELU6, name='stem')
    d = s.dwconv(x, 1, ns.SAME3, act=NONE, name='dw_1')
    t12 = s.conv(d, 12, 1, act=ns.LEAKY03, name='pw_1')
    t20 = s.conv(t12, 20, 1, act=ns.RELU, name='c1x1_12to20')
    t36 = s.conv(t12, 36, 3, act=ns.RELU6, name='c3x3_12to36')
    t100 = s.conv(t20, 100, 3, act=ns.LEAKY01, name='c3x3_20to100')
    t20b = s.conv(t36, 20, 1, act=NONE, name='c1x1_36to20')
    r = s.add(t20, t20b)
    q = s.maxpool(t20b, 1)
    s.conv(t100, 12, 1, act=ns.LEAKY01, name='c1x1_100to12')
    for t in (t12, t20, t36, t100):
        s.maxpool(t, 2)
    r2 = s.add(r, q)
    y = s.conv(r2, 18, 1, bn=False, bias=True, name='out', net_output=True)
    s.outputs = [y]
    return s, s.init_weights(seed=13)


def odd():
    """75x107 -> 38x54 -> 19x27 (odd) -> 10x14.
    Item 3: the stem and the frame maximum on an odd frame; on the 19x27 level a stride-2 pool (odd h and w), a stride-1 pool, a stride-2
    depthwise conv (fused with pw: 140 output pixels, ragged tiles) and a stride-2 3x3 conv.  Item 7: a 16-filter stem in front of a 3x3
    conv.  Item 1: Add(c3x3_s2, pw) folded into the fused block, and Add(r, c1x1_p2) with two convs between c1x1_p2 and the Add
    (standalone).  Item 6: an 18-channel output behind a fused 128-wide head, and one on the standalone Add."""
    s = ns.NetSpec('zoo_odd', (75, 107), anchor_num=3, class_num=1)
    x = s._new_tensor(75, 107, 3)
    x = s.conv(x, 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')                   # 38x54x16
    c1 = s.conv(x, 24, 3, act=ns.LEAKY01, name='c3x3_1')
    pl = s.maxpool(c1, 2)                                                                  # 19x27x24
    c2 = s.conv(pl, 32, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY01, name='c3x3_s2')              # 10x14x32
    p2 = s.maxpool(pl, 2)                                                                  # 10x14x24
    p1 = s.maxpool(pl, 1)                                                                  # 19x27x24
    d = s.dwconv(p1, 2, ns.K210_S2_PAD, act=ns.RELU, name='dw_s2')                         # 10x14x24
    pw = s.conv(d, 32, 1, act=NONE, name='pw')
    r = s.add(c2, pw)
    c3 = s.conv(p2, 32, 1, act=ns.LEAKY03, name='c1x1_p2')
    t = s.conv(r, 128, 3, act=ns.LEAKY01, name='head_mid')
    y1 = s.conv(t, 18, 1, bn=False, bias=True, name='head_out', net_output=True)
    r2 = s.add(r, c3)
    y2 = s.conv(r2, 18, 1, bn=False, bias=True, name='out_2', net_output=True)
    s.outputs = [y1, y2]
    return s, s.init_weights(seed=14)


ZOO = {'residual': residual, 'pyramid': pyramid, 'channels': channels, 'odd': odd}


# ---- graphs a plan must refuse: (name, what the f16x2 builder says, builder) -----------------------------------------
def _trunk(name, filters=16):
    """-> (spec, a: 8x12x32, b: 16x24x`filters` behind a 3x3 conv)."""
    s = ns.NetSpec(name, (32, 48), anchor_num=3, class_num=1)
    x = s._new_tensor(32, 48, 3)
    x = s.conv(x, 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')                   # 16x24x16
    b = s.conv(x, filters, 3, act=ns.LEAKY01, name='b')
    a = s.conv(b, 32, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY01, name='a')                      # 8x12x32
    return s, a, b


def _finish(s, t, net_output=True):
    y = s.conv(t, 18, 1, bn=False, bias=True, name='out', net_output=net_output)
    s.outputs = [y]
    return s, s.init_weights(seed=15)


def refuse_residual_zoo_spec():
    """tests/mini_net.py::residual_zoo_spec as the training tests use it: its head concatenates upsample(8 channels) in front"""
    s = residual_zoo_spec()
    return s, s.init_weights(seed=11)


def refuse_stem20():
    s = ns.NetSpec('refuse_stem20', (32, 48), anchor_num=3, class_num=1)
    x = s.conv(s._new_tensor(32, 48, 3), 20, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')
    return _finish(s, s.conv(x, 16, 1, act=ns.RELU, name='c'))


def refuse_concat24():
    s, a, b = _trunk('refuse_concat24', 24)
    b2 = s.conv(b, 16, 1, act=ns.RELU, name='b2')
    return _finish(s, s.conv(s.concat(b, b2), 16, 1, act=ns.RELU, name='c'))


def refuse_concat_up_second():
    s, a, b = _trunk('refuse_concat_up_second', 32)
    return _finish(s, s.conv(s.concat(b, s.upsample(a)), 16, 1, act=ns.RELU, name='c'))


def refuse_dw_on_upsample():
    s, a, b = _trunk('refuse_dw_on_upsample')
    return _finish(s, s.dwconv(s.upsample(a), 1, ns.SAME3, act=ns.RELU, name='dw'))


def refuse_dw_on_frame():
    s = ns.NetSpec('refuse_dw_on_frame', (32, 48), anchor_num=3, class_num=1)
    return _finish(s, s.dwconv(s._new_tensor(32, 48, 3), 1, ns.SAME3, act=ns.RELU, name='dw'))


def refuse_add_on_upsample():
    s, a, b = _trunk('refuse_add_on_upsample', 32)
    return _finish(s, s.add(s.upsample(a), b))


def refuse_pool_on_view():
    s, a, b = _trunk('refuse_pool_on_view')
    return _finish(s, s.maxpool(s.upsample(a), 2))


def refuse_output_not_flagged():
    s, a, b = _trunk('refuse_output_not_flagged')
    return _finish(s, a, net_output=False)


REFUSALS = [
    (refuse_residual_zoo_spec, 'multiples of 32'),
    (refuse_stem20, 'stem conv must be 3x3 with 16/24/32 filters'),
    (refuse_concat24, 'multiples of 32'),
    (refuse_concat_up_second, 'unsupported input view nesting'),
    (refuse_dw_on_upsample, 'depthwise conv on a view/input'),
    (refuse_dw_on_frame, 'depthwise conv on a view/input'),
    (refuse_add_on_upsample, 'standalone Add on views'),
    (refuse_pool_on_view, 'max pool on a view/input'),
    (refuse_output_not_flagged, 'not produced by a NET_OUTPUT conv'),
]
