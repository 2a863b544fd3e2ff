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
  8 activations  depthwise + LeakyReLU(0.1), depthwise without activation, pointwise + ReLU, 3x3 + ReLU6

CLUSTER_ZOO (further down) is a second set, for the latency schedule's two cluster launches x:persist[...] and x:heads[...]: each spec
holds one chain of depthwise + pointwise launches and a trailing run of convs chosen so that, between them, they reach the kernel
instantiations and phase shapes that yolo_mobilev1 0.75 at 224x320 - the one network held to the strict criterion in that schedule -
leaves out (CLUSTER_TARGETS).  persist_plan / heads_plan restate the builders' integer rules to say which those are."""
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
        if i >= len(self.ops):
            return None
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


# ---- the latency schedule's two cluster launches: the builder's rules restated, and specs that reach what yolo_mobilev1 does not ----
XP_CW, XP_MAXPH, XP_YB_BYTES, XP_RING_CAP, XP_RESIDENT = 8, 24, 68 * 1024, 3 * 8 * 6 * 1024, 76 * 1024     # yk_xpersist.h:32,500; yk_exact.hip:1186,1279
XH_CW, XH_MAXPH, XH_NCH = 8, 6, 3                                                                         # yk_xheads.h:28


def latency_launches(spec):
    """The f16x2 latency plan's launch list in front of x_build_persist / x_build_heads, as far as they look at it: [(kind, op index)],
    kind 'dw' (a depthwise launch of its own), 'conv' (XK_CONV) or 'other'.  emit() goes through the ops in order; views and folded Adds
    emit nothing; decide_blocks (yk_xplan_build.h:145-178) turns a depthwise conv + 1x1 conv into one XK_BLOCK launch from 128 output
    pixels on and, with the persistent stage on, up to max_nk = 6 steps of 32 input channels; the heads launch switches the fused heads
    off (x_read_opts, :21), so every other conv but the stem is an XK_CONV launch."""
    g = Graph(spec)
    out = []
    for i, op in enumerate(spec.ops):
        ty = op['type']
        if ty in VIEWS or (ty == ns.OP_ADD and g.folded_add(i) is not None):
            continue
        fused = lambda k: g.dw_fused(k) and (spec.ops[k]['cin'] + 31) // 32 <= 6          # noqa: E731
        if ty == ns.OP_DWCONV:
            if not fused(i):
                out.append(('dw', i))
        elif ty == ns.OP_CONV and op['in0'] != 0 and not (i > 0 and spec.ops[i - 1]['type'] == ns.OP_DWCONV and fused(i - 1)):
            out.append(('conv', i))
        else:
            out.append(('other', i))
    return out


def persist_plan(spec):
    """x_build_persist (yk_exact.hip:1184-1369) restated over spec.ops -> None where no chain is taken, else a dict:
      blocks   one per depthwise + pointwise pair: nrb, ncb, adirect, resident, ppw, WR, WC, zero_border (the pointwise phase's fields),
               after_direct (the adirect of the pointwise phase in front of it in the chain), pad (the depthwise conv's), store (an
               XP_STORE phase follows), and the op index of the depthwise conv
      src_f32  the chain's input is stored as fp32 planes (mark_f32_planes, yk_xplan_build.h:782-812)
      name     the prefix of the launch name
    The copy can drift from the C++ in the choice of a variant; what the launch name carries - block count, start shape, phase count,
    barrier count - is what tests/test_gpu_plan_zoo.py asserts against the builder itself."""
    g, L = Graph(spec), latency_launches(spec)
    ops = spec.ops

    def dw_ok(k):                                                       # :1192
        return k < len(L) and L[k][0] == 'dw' and ops[L[k][1]]['cin'] % 64 == 0

    def pw_ok(k):                                                       # :1187-1191; splitk == 1: x_conv_tiling (yk_xplan_build.h:57) splits K from 32
        if k >= len(L) or L[k][0] != 'conv':                            # steps of 32 channels on while the grid has < 384 tiles (any zoo frame)
            return False
        i, o = L[k][1], ops[L[k][1]]
        return (o['k'] == 1 and o['stride'] == 1 and g.kind(o['in0']) not in VIEWS and g.folded_add(i + 1) != i and
                (o['cin'] + 31) // 32 < 32 and not (o['flags'] & ns.FLAG_NET_OUTPUT) and o['cout'] % (16 * XP_CW) == 0 and o['cin'] % 64 == 0)

    def y_fits(h, w_, gs):                                              # :1193
        return 2 * (h + 2) * (w_ + 2) * gs * 16 <= XP_RING_CAP

    best = None
    i = 0
    while i < len(L):                                                   # :1196-1216
        blocks = 0
        if dw_ok(i):
            k = i
            while dw_ok(k) and pw_ok(k + 1) and ops[L[k + 1][1]]['in0'] == ops[L[k][1]]['out'] and g.uses[ops[L[k][1]]['out']] == 1:
                d, q = ops[L[k][1]], ops[L[k + 1][1]]
                hi, wi, _ = g.shape(d['in0'])
                ho, wo, _ = g.shape(d['out'])
                nrb, ncb = (ho * wo + 15) // 16, q['cout'] // 16 // XP_CW
                ok = 2 * (nrb + ncb) <= 48 and y_fits(hi, wi, d['cin'] // 64) and y_fits(ho, wo, q['cout'] // 64) and hi * wi <= 1024
                tile = any((nrb + wr - 1) // wr <= 3 and (ncb + 8 // wr - 1) // (8 // wr) <= 3 for wr in (8, 4, 2, 1))
                if not (ok and tile):
                    break
                blocks += 1
                k += 2
                if not (dw_ok(k) and ops[L[k][1]]['in0'] == q['out']):
                    break
            if blocks >= 2 and (best is None or blocks > best[1]):
                best = (i, blocks)
        i += 2 * blocks if blocks else 1
    if best is None:
        return None
    first, nblocks = best
    out, prev, nstore = [], None, 0
    for b in range(nblocks):
        d, q = ops[L[first + 2 * b][1]], ops[L[first + 2 * b + 1][1]]
        ho, wo, _ = g.shape(d['out'])
        r = dict(op=L[first + 2 * b][1], H=ho, W=wo, cin=d['cin'], n=q['cout'], pad=g.pad(d), stride=d['stride'], acts=(d['act'], q['act']))
        r['nrb'], r['ncb'], nks, gs = (ho * wo + 15) // 16, q['cout'] // 16 // XP_CW, d['cin'] // 32, q['cout'] // 64
        bt = 100
        for wr in (8, 4, 2, 1):                                         # :1265-1272
            tr, tc = (r['nrb'] + wr - 1) // wr, (r['ncb'] + 8 // wr - 1) // (8 // wr)
            if tr <= 3 and tc <= 3 and tr * tc < bt:
                bt, r['WR'], r['WC'] = tr * tc, wr, 8 // wr
        r['ppw'] = max(3, (2 * (r['nrb'] + r['ncb']) + 7) // 8)         # :1273
        ad = res = 0
        if 2 * (ho + 2) * (wo + 2) * gs * 16 <= XP_YB_BYTES:            # :1276-1282, branch for branch
            if r['nrb'] <= 24 and r['ncb'] == 3:
                ad = 1
            elif r['nrb'] <= 24 and r['ncb'] == 2:
                ad = 3
            if ad in (1, 3) and nks * r['ncb'] * 2048 <= XP_RESIDENT:
                res = 1
            elif r['nrb'] == 5 and r['ncb'] <= 8:
                ad = 2
            elif r['nrb'] == 5 and r['ncb'] <= 16:
                ad = 4
        r['adirect'], r['resident'] = ad, res
        shape = (ho, wo, gs)
        if prev is None:                                                # :1314-1322: the LOAD phase's shape stands in front of the first block
            hi, wi, _ = g.shape(d['in0'])
            prev = ((hi, wi, d['cin'] // 64), 0)
        r['zero_border'] = int(not (ad and shape == prev[0]))
        r['after_direct'] = prev[1]
        prev = (shape, ad)
        r['store'] = b == nblocks - 1 or g.uses[q['out']] != 1          # :1293-1303
        nstore += r['store']
        out.append(r)
    nph = 1 + 2 * nblocks + nstore
    if nph > XP_MAXPH:                                                  # :1305
        return None
    t0 = ops[L[first][1]]['in0']
    hi, wi, ci = g.shape(t0)
    src_f32 = g.uses[t0] == 1 and g.kind(t0) == ns.OP_CONV and g.folded_add(g.producer[t0] + 1) is None and t0 not in spec.outputs
    return dict(blocks=out, src_f32=src_f32, first=first, name=f'x:persist[{nblocks} blocks dw3x3+conv1x1 from {hi}x{wi}x{ci},{nph} phases,'
                f'{nblocks} cluster barriers,{XP_CW} wg/image]')


def heads_plan(spec):
    """x_build_heads / x_build_heads_from (yk_exact.hip:1376-1518) restated -> None, or a dict: phases (in the launch's order: conv, the op
    index, variant, nrb, ncb, nchunk, tail = the output conv's channel count or 0, pre_barrier, up, cat) and name, the launch name.  The
    trailing run of conv launches is taken after the persistent launch has replaced its chain, which never is part of that run.  As in
    persist_plan, the variant is this copy's; the phase list and the barrier count are in the launch name."""
    g, L, ops = Graph(spec), latency_launches(spec), spec.ops
    first = len(L)
    while first > 0 and L[first - 1][0] == 'conv':                      # :1379
        first -= 1

    def conv_ok(o):                                                     # :1390-1393
        return (o['stride'] == 1 and g.shape(o['out'])[:2] == g.shape(o['in0'])[:2] and
                ((o['k'] == 1 and o['pad_t'] == 0 and o['pad_l'] == 0) or (o['k'] == 3 and o['pad_t'] == 1 and o['pad_l'] == 1)))

    def label(o):
        view = '+upcat' if g.kind(o['in0']) == ns.OP_CONCAT else '+up' if g.kind(o['in0']) == ns.OP_UPSAMPLE else ''
        return f'conv{o["k"]}x{o["k"]}s1_{o["cin"]}to{o["cout"]}{view}'

    def build(first):
        ph, k, lds = [], first, 0
        while k < len(L):
            i, o = L[k][1], ops[L[k][1]]
            if not conv_ok(o) or g.folded_add(i + 1) == i or (o['flags'] & ns.FLAG_NET_OUTPUT) or o['cout'] % 16:      # :1405
                return None
            srcs, up = [o['in0']], 0
            if g.kind(o['in0']) == ns.OP_CONCAT:
                srcs = [g.prod(o['in0'])['in0'], g.prod(o['in0'])['in1']]
            if g.kind(srcs[0]) == ns.OP_UPSAMPLE:
                srcs[0], up = g.prod(srcs[0])['in0'], 1
            h, w_, _ = g.shape(o['out'])
            q = dict(op=i, taps=o['k'] ** 2, nrb=(h * w_ + 15) // 16, ncb=o['cout'] // 16, up=up, cat=len(srcs) == 2, srcs=srcs, out=o['out'],
                     nchunk=sum(((g.shape(t)[2] + 7) // 8 + 3) // 4 for t in srcs), tail=0, pre_barrier=0, name=label(o))
            pp = (h + 2) * (w_ + 2)
            if pp > 384:                                                # :1420
                return None
            if q['taps'] == 9 and q['nrb'] <= 5 and q['ncb'] <= 12 and q['nchunk'] <= 24 and not q['cat']:               # :1421-1424
                q['variant'], wk = 1, 2
            elif q['taps'] == 9 and q['nrb'] <= 18 and q['ncb'] <= 8 and q['nchunk'] <= 16:
                q['variant'], wk = 0, 1
            elif q['taps'] == 1 and q['nrb'] <= 5 and q['ncb'] <= 8 and q['nchunk'] <= 24 and not q['cat']:
                q['variant'], wk = 2, 2
            else:
                return None
            lds = max(lds, min(XH_NCH, (q['nchunk'] + XH_CW - 1) // XH_CW) * 2 * pp * 64)
            if wk == 2:
                lds = max(lds, q['nrb'] * q['ncb'] * 1024)
            t = ops[L[k + 1][1]] if k + 1 < len(L) else None
            if (t and (t['flags'] & ns.FLAG_NET_OUTPUT) and t['k'] == 1 and conv_ok(t) and t['in0'] == o['out'] and
                    g.uses[o['out']] == 1):                             # :1435-1436
                t_nks, t_ncb = ((o['cout'] + 7) // 8 + 3) // 4, (t['cout'] + 15) // 16
                t_nslab = (t['cout'] + 63) // 64 * 4                    # a 64-wide tile below 256 tiles (x_conv_tiling), 128-wide: no fewer
                if t_nks * 32 < q['ncb'] * 16 or t_ncb > t_nslab or t_nks > 6:      # :1442
                    return None
                lds = max(lds, 48 * (q['ncb'] * 16 + 4) * 4 + 64)
                q['tail'], q['out'] = t['cout'], None
                q['name'] += f'+conv1x1s1_{t["cin"]}to{t["cout"]}'
                k += 1
            ph.append(q)
            k += 1
        if not ph or len(ph) > XH_MAXPH or lds + 256 > 156 * 1024:      # :1452-1453
            return None

        def feeds(x):
            return int(x['out'] is not None and any(x['out'] in y['srcs'] for y in ph))
        rank = [feeds(x) for x in ph]
        ph = [x for r, x in sorted(zip(rank, ph), key=lambda rx: -rx[0])]      # :1455-1463 (stable, feeders first)
        for n, q in enumerate(ph):                                      # :1465-1477
            for m, y in enumerate(ph):
                if y['out'] is not None and y['out'] in q['srcs']:
                    if m >= n:
                        return None
                    if m + 1 == n:
                        q['pre_barrier'] = 1
        if len(ph) == 1:
            ph[0]['pre_barrier'] = 1
        return ph
    while len(L) - first >= 2:                                          # :1381-1385
        ph = build(first)
        if ph:
            nbar = sum(1 + q['pre_barrier'] for q in ph)
            return dict(phases=ph, name='x:heads[' + ' | '.join(q['name'] for q in ph) + f';K split over {XH_CW} wg/image,{nbar} cluster barriers]')
        first += 1
    return None


def cluster_targets(spec):
    """Which of the paths of the two cluster launches that yolo_mobilev1 0.75 at 224x320 leaves out a spec's latency plan reaches
    (persist_plan, heads_plan) -> set of names.  tests/test_plan_zoo.py holds the union over CLUSTER_ZOO against CLUSTER_TARGETS."""
    hit = set()
    p, h = persist_plan(spec), heads_plan(spec)
    if p:
        hit.add('chain from fp32 planes' if p['src_f32'] else 'chain from a split tensor')
        for n, b in enumerate(p['blocks']):
            res = 'resident' if b['resident'] else 'non-resident'
            if b['adirect'] == 0:
                hit.add(f'ring ppw {min(b["ppw"], 6)}')
            elif b['adirect'] in (1, 3):
                hit.add(f'adirect {b["adirect"]} {res}')
                hit.add(f'adirect {b["adirect"]} {res} nrb {b["nrb"]}' + (' ragged' if (b['H'] * b['W']) % 16 else ''))
            elif b['adirect'] == 2:
                hit.add(f'adirect 2 ncb {b["ncb"]}')
                if b['ncb'] in (2, 3):
                    hit.add('adirect 2 through the fall-through')
            else:
                hit.add('adirect 4')
            hit.add(f'tiling {b["WR"]}x{b["WC"]}')
            if b['stride'] == 2:
                hit.add(f'stride 2 pad {b["pad"]}')
            hit.add(f'dw act {b["acts"][0]}')
            hit.add(f'pw act {b["acts"][1]}')
            if b['store'] and n + 1 < len(p['blocks']):
                hit.add(f'mid-chain store behind adirect {b["adirect"]}')
            if b['after_direct'] and b['zero_border']:
                hit.add(f'shape change behind adirect {b["after_direct"]} into ' + (f'adirect {b["adirect"]}' if b['adirect'] else 'the ring form'))
    if h:
        if len(h['phases']) == 1:
            hit.add('heads: single phase')
        for q in h['phases']:
            v = q['variant']
            if q['nchunk'] < XH_CW:
                hit.add(f'heads: variant {v} with idle members')
            hit.add(f'heads: variant {v} nrb {q["nrb"]}')
            if q['ncb'] % 4:
                hit.add(f'heads: variant {v} ncb % 4')
            if q['pre_barrier'] and len(h['phases']) > 1:
                hit.add('heads: pre_barrier by adjacency')
            if v == 2 and q['up']:
                hit.add('heads: 1x1 on an upsample view')
            if v == 2 and q['nchunk'] == 2 and q['ncb'] == 1:
                hit.add('heads: 1x1 64 -> 16')
            if v == 1 and q['nrb'] < 5 and q['ncb'] in (3, 5):
                hit.add('heads: variant 1 small with a tail' if q['tail'] else 'heads: variant 1 small without a tail')
            if v == 0 and 6 <= q['nrb'] <= 17 and q['cat'] and q['up']:
                hit.add('heads: variant 0 nrb 6..17 on concat(upsample, b)')
            if v == 0 and 9 <= q['nchunk'] <= 15:
                hit.add('heads: variant 0 nchunk 9..15')
            if q['tail']:
                hit.add(f'heads: tail {q["ncb"] * 16} -> {q["tail"]}' + (' behind a 1x1' if v == 2 else ''))
    return hit


CLUSTER_TARGETS = {
    'ring ppw 3', 'ring ppw 4', 'ring ppw 5', 'ring ppw 6',
    'adirect 1 resident nrb 9 ragged', 'adirect 1 non-resident', 'adirect 3 resident', 'adirect 3 non-resident',
    'adirect 2 ncb 1', 'adirect 2 ncb 8', 'adirect 2 through the fall-through', 'adirect 4',
    'tiling 2x4', 'tiling 1x8',
    f'stride 2 pad {KERAS_SAME_S2}', f'stride 2 pad {DARKNET_S2}',
    f'dw act {ns.ACT_LEAKY}', f'dw act {ns.ACT_RELU6}', f'dw act {ns.ACT_NONE}',
    f'pw act {ns.ACT_RELU6}', f'pw act {ns.ACT_NONE}',
    'chain from a split tensor', 'mid-chain store behind adirect 2',
    'shape change behind adirect 2 into adirect 2', 'shape change behind adirect 2 into adirect 4',
    'shape change behind adirect 1 into the ring form', 'shape change behind adirect 3 into the ring form',
    'heads: variant 2 with idle members', 'heads: variant 1 with idle members', 'heads: variant 0 with idle members',
    'heads: variant 0 nrb 6', 'heads: variant 0 nrb 9', 'heads: variant 1 nrb 3', 'heads: variant 2 nrb 3',
    'heads: variant 1 ncb % 4', 'heads: variant 2 ncb % 4',
    'heads: pre_barrier by adjacency', 'heads: single phase', 'heads: 1x1 on an upsample view', 'heads: 1x1 64 -> 16',
    'heads: variant 1 small with a tail', 'heads: variant 1 small without a tail',
    'heads: variant 0 nrb 6..17 on concat(upsample, b)', 'heads: variant 0 nchunk 9..15',
    'heads: tail 128 -> 18', 'heads: tail 128 -> 80', 'heads: tail 48 -> 18', 'heads: tail 64 -> 18 behind a 1x1',
}


def _chain(s, x, blocks):
    """depthwise + pointwise blocks (stride, pad, depthwise act, filters, pointwise act) -> the pointwise outputs.  Behind the chain a
    stride-2 pool reads every pointwise output but the last: a second reader, so the persistent launch stores it (XP_STORE; the next
    block still reads it from LDS) and the layerwise check holds each block to a bound from the block in front of it.  A bound that
    spans two blocks is some 400 times wider than the error (error / E = 0.002): a dropped hi x lo product stayed below it (0.89)."""
    outs = []
    for n, (stride, pad, dact, f, pact) in enumerate(blocks, start=1):
        x = s.conv(s.dwconv(x, stride, pad, act=dact, name=f'dw_{n}'), f, 1, act=pact, name=f'pw_{n}')
        outs.append(x)
    for t in outs[:-1]:
        s.maxpool(t, 2)
    return outs


def cluster_wide():
    """64x80 -> 32x40 -> 16x20, the chain goes on to 8x10 (80 pixels: nrb 5).  The chain's input (16x20x256, behind a plain stride-2 3x3
    conv) has the first depthwise conv as its only reader: fp32 planes.
      pw_1  256 -> 128 at 16x20   ring form, ppw 6 (nrb 20, ncb 1); 320 pixels, kept out of a fused block by its 8 steps of 32 channels
      dw_2  stride 2, pad (0, 1, 0, 1), LeakyReLU(0.1)
      pw_2  128 -> 128 at 8x10    adirect 2 with ncb 1; head_mid reads its output too: a heads phase on a tensor the persistent launch stored
      pw_3  128 -> 640            adirect 2, ncb 5: a shape change (Gs 2 -> 10) directly behind a direct phase; ReLU6
      pw_4  640 -> 256            ncb 2 and 80 KB of weights: adirect 3, not resident, nrb 5 -> the fall-through makes it adirect 2
      pw_5  256 -> 1024           adirect 2 with ncb 8 (tiling 2x4); 1024 channels end the chain (a K-split conv behind it)
    Heads: wide (1x1 on 1024 channels: 32 chunks) stays a launch in front; pre_mid 128 -> 64 (variant 2, 4 chunks) is stored and read by
    pre_out 64 -> 16 (variant 2: 2 chunks, six idle members, ncb 1) right behind it: pre_barrier by adjacency; head_mid (3x3 on pw_2's
    stored output, variant 1, ncb 12) + head_out 192 -> 75."""
    s = ns.NetSpec('zoo_cluster_wide', (64, 80), anchor_num=3, class_num=20)
    x = s.conv(s._new_tensor(64, 80, 3), 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')           # 32x40x16
    x = s.conv(x, 256, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY01, name='down')                                  # 16x20x256
    p = _chain(s, x, [(1, ns.SAME3, ns.RELU, 128, ns.LEAKY03), (2, KERAS_SAME_S2, ns.LEAKY01, 128, ns.LEAKY03),
                      (1, ns.SAME3, ns.RELU6, 640, ns.RELU6), (1, ns.SAME3, NONE, 256, ns.LEAKY03), (1, ns.SAME3, ns.RELU, 1024, NONE)])
    c = s.conv(p[4], 128, 1, act=ns.LEAKY01, name='wide')
    m = s.conv(c, 64, 1, act=ns.RELU, name='pre_mid')
    s.conv(m, 16, 1, act=ns.LEAKY01, name='pre_out')
    t = s.conv(p[1], 192, 3, act=ns.LEAKY01, name='head_mid')
    y = s.conv(t, 75, 1, bn=False, bias=True, name='head_out', net_output=True)
    s.outputs = [y]
    return s, s.init_weights(seed=21)


def cluster_ragged():
    """40x56 -> 20x28 -> 10x14 (140 pixels: nrb 9, a ragged last block), the chain goes on to 5x7 (nrb 3).  The chain's input has a second
    reader (head_mid through its concat): stored as (hi | lo).
      pw_1  256 -> 384 at 10x14   adirect 1, resident, ragged
      pw_2  384 -> 512            ring form, ppw 4 (nrb 9 + ncb 4 = 13), no activation on either half
      pw_3  512 -> 384            adirect 1 with 96 KB of weights: not resident (nrb != 5: stays adirect 1)
      dw_4  stride 2, pad (1, 0, 1, 0)
      pw_4  384 -> 640 at 5x7     ring form, ppw 3, behind a direct phase with another shape
      pw_5  640 -> 256            adirect 3 with 80 KB of weights: not resident
      pw_6  256 -> 1024           ring form, nrb 3 x ncb 8: the 1x8 tiling
    Heads: wide stays a launch in front; up_mid 128 -> 64 at 5x7 is stored; small_mid (3x3, variant 1, nrb 3, ncb 3, 4 chunks) + small_out
    48 -> 18; small_open (3x3, variant 1, ncb 5) without a tail; head_mid = 3x3 on concat(upsample(up_mid), chain input), variant 0 at
    nrb 9 with 2 + 8 = 10 chunks, two phases behind up_mid (no pre_barrier) + head_out 128 -> 80."""
    s = ns.NetSpec('zoo_cluster_ragged', (40, 56), anchor_num=5, class_num=11)
    x = s.conv(s._new_tensor(40, 56, 3), 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')           # 20x28x16
    x = s.conv(x, 256, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY01, name='down')                                  # 10x14x256
    p = _chain(s, x, [(1, ns.SAME3, ns.RELU, 384, ns.LEAKY03), (1, ns.SAME3, NONE, 512, NONE), (1, ns.SAME3, ns.RELU, 384, ns.RELU6),
                      (2, DARKNET_S2, ns.RELU6, 640, ns.LEAKY03), (1, ns.SAME3, ns.LEAKY01, 256, ns.LEAKY03),
                      (1, ns.SAME3, ns.RELU, 1024, ns.LEAKY03)])
    c = s.conv(p[5], 128, 1, act=ns.LEAKY01, name='wide')                                                  # 5x7x128
    u = s.conv(c, 64, 1, act=ns.LEAKY01, name='up_mid')
    t = s.conv(c, 48, 3, act=ns.LEAKY01, name='small_mid')
    y1 = s.conv(t, 18, 1, bn=False, bias=True, name='small_out', net_output=True)
    s.conv(c, 80, 3, act=ns.RELU, name='small_open')
    t = s.conv(s.concat(s.upsample(u), x), 128, 3, act=ns.LEAKY01, name='head_mid')                        # 10x14, 64 + 256 channels
    y2 = s.conv(t, 80, 1, bn=False, bias=True, name='head_out', net_output=True)
    s.outputs = [y1, y2]
    return s, s.init_weights(seed=22)


def cluster_ring():
    """32x48 -> 16x24 -> 8x12 (96 pixels: nrb 6); the chain stays there and starts from fp32 planes.
      pw_1  64 -> 128     ring form, ppw 3 (nrb 6, ncb 1); 64 input channels, kept out of a fused block by its 96 pixels
      pw_2  128 -> 256    adirect 3, resident
      pw_3  256 -> 1536   ring form, ppw 5 (nrb 6 + ncb 12 = 18), the 2x4 tiling, behind a direct phase with another shape
    Heads: wide stays a launch in front; the launch is head_mid (3x3, variant 0: nrb 6 > 5, 4 chunks) + head_out 128 -> 18 alone: a
    single phase."""
    s = ns.NetSpec('zoo_cluster_ring', (32, 48), anchor_num=3, class_num=1)
    x = s.conv(s._new_tensor(32, 48, 3), 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')           # 16x24x16
    x = s.conv(x, 64, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY01, name='down')                                   # 8x12x64
    p = _chain(s, x, [(1, ns.SAME3, ns.LEAKY01, 128, ns.RELU6), (1, ns.SAME3, ns.RELU, 256, NONE), (1, ns.SAME3, NONE, 1536, ns.LEAKY03)])
    c = s.conv(p[2], 128, 1, act=ns.LEAKY01, name='wide')
    t = s.conv(c, 128, 3, act=ns.LEAKY01, name='head_mid')
    y = s.conv(t, 18, 1, bn=False, bias=True, name='head_out', net_output=True)
    s.outputs = [y]
    return s, s.init_weights(seed=23)


def cluster_deep():
    """56x80 -> 28x40 -> 14x20 -> 7x10 (70 pixels: nrb 5, ragged); the chain stays there and starts from fp32 planes of 448 channels.
      pw_1  448 -> 384    ncb 3 and 84 KB of weights: adirect 1, not resident, nrb 5 -> the fall-through makes it adirect 2
      pw_2  384 -> 128    adirect 2 with ncb 1
      pw_3  128 -> 1280   adirect 4 (ncb 10), the 2x4 tiling; 1152 and 1280 are the widths whose y image fits 68 KB here
    Heads: wide stays a launch in front, and a pool of it (4x5) goes in front of the convs; up_only = 1x1 on upsample(pool) alone at 8x10
    (variant 2); flat_mid (1x1, variant 2) + flat_out 64 -> 18: a tail behind a 1x1 phase; head_mid (3x3, variant 1 at nrb 5, ncb 8) +
    head_out 128 -> 18."""
    s = ns.NetSpec('zoo_cluster_deep', (56, 80), anchor_num=3, class_num=1)
    x = s.conv(s._new_tensor(56, 80, 3), 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='stem')           # 28x40x16
    x = s.conv(x, 32, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY01, name='down_1')                                 # 14x20x32
    x = s.conv(x, 448, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY01, name='down_2')                                # 7x10x448
    p = _chain(s, x, [(1, ns.SAME3, ns.RELU, 384, ns.LEAKY03), (1, ns.SAME3, ns.LEAKY01, 128, ns.RELU6), (1, ns.SAME3, ns.RELU6, 1280, ns.LEAKY03)])
    c = s.conv(p[2], 128, 1, act=ns.LEAKY01, name='wide')
    q = s.maxpool(c, 2)                                                                                    # 4x5x128
    s.conv(s.upsample(q), 32, 1, act=ns.LEAKY01, name='up_only')                                           # 8x10x32
    t = s.conv(c, 64, 1, act=ns.LEAKY01, name='flat_mid')
    y1 = s.conv(t, 18, 1, bn=False, bias=True, name='flat_out', net_output=True)
    t = s.conv(c, 128, 3, act=ns.LEAKY01, name='head_mid')
    y2 = s.conv(t, 18, 1, bn=False, bias=True, name='head_out', net_output=True)
    s.outputs = [y1, y2]
    return s, s.init_weights(seed=24)


CLUSTER_ZOO = {'cluster_wide': cluster_wide, 'cluster_ragged': cluster_ragged, 'cluster_ring': cluster_ring, 'cluster_deep': cluster_deep}


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
