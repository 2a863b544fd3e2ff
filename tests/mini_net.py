"""Small detectors for the tests.  mini_spec: the layer kinds and NAMES the reference's Keras models use (shared by
tests/golden/make_h5_golden.py, which runs under an interpreter with h5py, and tests/test_h5lite.py).  residual_zoo_spec: residual
wiring for the training tests."""
from k210_yolo_framework_amd import netspec as ns


def mini_spec(class_num=20):
    """conv1 -> 2 x (depthwise + pointwise) -> the y1/y2 head pattern of yolonet.py:27-38, 8..32 channels."""
    s = ns.NetSpec('mini', (32, 32), anchor_num=3, class_num=class_num)
    x = s._new_tensor(32, 32, 3)
    x = s.conv(x, 8, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='conv1')
    x = s.dwconv(x, 1, ns.SAME3, act=ns.RELU, name='conv_dw_1')
    x1 = s.conv(x, 16, 1, act=ns.LEAKY03, name='conv_pw_1')
    x = s.dwconv(x1, 2, ns.K210_S2_PAD, act=ns.RELU, name='conv_dw_2')
    x = s.conv(x, 32, 1, act=ns.LEAKY03, name='conv_pw_2')
    ns._head(s, x1, x, 24, 16, 8, 3 * (class_num + 5), [0])
    return s


def residual_zoo_spec():
    """Residual wiring the reference networks do NOT use (NetSpec is a general builder): Add(conv_out, shortcut) with the operands swapped,
    an Add whose input is another Add's output, a shortcut read by three consumers, and a linear (no-BN) conv feeding an Add."""
    s = ns.NetSpec('zoo', (32, 48), anchor_num=3, class_num=20)
    x = s._new_tensor(32, 48, 3)
    x = s.conv(x, 16, 3, 2, ns.K210_S2_PAD, act=ns.LEAKY03, name='conv1')
    a = s.conv(x, 16, 1, act=ns.RELU6, name='conv_a')
    r1 = s.add(a, x)                                       # operands swapped: (conv output, shortcut)
    b = s.conv(r1, 16, 1, act=ns.LEAKY03, name='conv_b')
    r2 = s.add(r1, b)                                      # the usual order
    r3 = s.add(r2, r1)                                     # nested: r2 is itself an Add; r1 now has three readers
    c = s.conv(r3, 16, 1, bn=False, bias=True, name='conv_c')   # no BatchNorm: its backward hands dy on as dz
    r4 = s.add(r3, c)
    x1 = s.conv(r4, 16, 1, act=ns.LEAKY03, name='conv_pw_1')
    t = s.dwconv(x1, 2, ns.K210_S2_PAD, act=ns.RELU, name='conv_dw_2')
    x2 = s.conv(t, 32, 1, act=ns.LEAKY03, name='conv_pw_2')
    ns._head(s, x1, x2, 24, 16, 8, 75, [0])
    return s
