"""The launch-at-a-time checkers of the two inference plans, shared by tests/test_gpu_layers_x2.py, tests/test_gpu_layers.py and
tests/test_gpu_plan_zoo.py.  What they assert is described in the first two of those files; nothing here is specific to a network."""
import contextlib
import os
import re
import time

import numpy as np

import oracle
from k210_yolo_framework_amd import netspec as ns
from oracle import x2_bound as xb

SWITCHES = ('YK_FUSE_DWPW', 'YK_SPLITK', 'YK_FUSE_HEAD', 'YK_CLUSTER_WT')


@contextlib.contextmanager
def _switches(env=None):
    """The plan switches a plan builder samples from the environment, for the plans created inside: all unset (the defaults) but those in
    `env`; whatever the process held before comes back afterwards, so no test's plan depends on the tests that ran before it."""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env or {})
    try:
        yield
    finally:
        for k in set(SWITCHES) | set(env or {}):
            os.environ.pop(k, None)
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v


def _frames(spec, B, seed):
    """Random u8 frames; per batch one dark image (// 20), one whose maximum is below 255, one with a saturated block over a dim rest:
    the per-image exponents differ inside a batch."""
    H, W = spec.in_hw
    f = np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    f[0] //= 20
    k = 1 % B
    f[k] = np.minimum(f[k], 200)
    k = 2 % B
    top = int(f[k].max())
    f[k] //= 3
    f[k, H // 4:H // 2, W // 4:W // 2] = top
    return f


def _stored_outputs(name):
    """How many tensors a launch leaves in memory, from its name in the launch list."""
    if name == 'u8_max':
        return 0
    if name.startswith('x:heads['):
        return name.count(' | ') + 1                                  # every phase stores its tensor or the output of its 1x1 tail
    m = re.match(r'x:persist\[(\d+) blocks.*?,(\d+) phases', name)
    if m:
        return int(m.group(2)) - 1 - 2 * int(m.group(1))              # phases = load + (dw, pw) per block + stores
    return 1


def _layerwise(spec, w, B, schedule='throughput', env=None, f32_entry=False, seed=0):
    """f16x2 -> (launch names, [(launch name, tensor, op index, error / E)], worst over-estimate)."""
    import torch
    from k210_yolo_framework_amd import engine
    with _switches(env):
        frames = _frames(spec, B, seed)
        plan = engine.Plan(spec, w, max_batch=B, precision='f16x2', schedule=schedule)
        x0 = frames.astype(np.float64) / frames.reshape(B, -1).max(1).astype(np.float64).reshape(B, 1, 1, 1)
        if f32_entry:
            x32 = x0.astype(np.float32)
            x0 = x32.astype(np.float64)
            plan.run_f32(torch.from_numpy(x32).cuda())
        else:
            plan.run_u8(torch.from_numpy(frames).cuda())
        plan.check()
        gpu, fmt = {0: x0}, {}
        readers = {}
        for op in spec.ops:
            for t in (op['in0'], op['in1']):
                if t >= 0:
                    readers.setdefault(t, []).append(op['type'])
        over = 0.0
        for op in spec.ops:
            t = op['out']
            if op['type'] in (ns.OP_UPSAMPLE, ns.OP_CONCAT):
                continue                                               # views: a consumer reads their sources
            try:
                v = plan.read_tensor(t, B)
            except engine.YkError as e:
                if 'fused away' in str(e) or 'folded away' in str(e):
                    continue                                           # lives only in LDS / registers
                raise
            assert np.isfinite(v).all(), f'tensor {t} ({op.get("layer")}): non-finite read-back'
            gpu[t] = v
            if t in spec.outputs:
                fmt[t] = ('f32',)
                continue
            e = plan.read_exponents(t, B)
            if readers.get(t) == [ns.OP_DWCONV] and not e.any() and not xb.is_split(v, e).all():
                fmt[t] = ('f32',)                                      # fp32 planes: exponent 0 and values no (hi, lo) pair can hold
                continue
            ok, o, msg = xb.split_health(v, e)
            assert ok, f'tensor {t} ({op.get("layer")}): {msg}; exponents {e.tolist()}'
            assert xb.is_split(v, e).all(), f'tensor {t} ({op.get("layer")}): a read-back value is not hi + lo at its exponent'
            over = max(over, o)
            fmt[t] = ('split', e)
        names = [l[0] for l in plan.launches()]
        plan.close()
    expect = sum(_stored_outputs(n) for n in names)
    stored = [op['out'] for op in spec.ops if op['out'] in fmt]
    assert len(stored) == expect, (f'{expect} stored tensors according to the launch list, {len(stored)} could be read', names)
    owner = [n for n in names for _ in range(_stored_outputs(n))]       # launches and stored tensors both come in issue order
    producer = {op['out']: i for i, op in enumerate(spec.ops)}
    rows = []
    for name, t in zip(owner, stored):
        idx, ins = xb.launch_chain(spec, set(gpu), t)
        f = {t: fmt[t]}
        for i in idx[:-1]:                                             # inner tensors an in-chain conv reads: split at an unstored exponent
            o = spec.ops[i]
            if o['type'] in (ns.OP_CONV, ns.OP_DWCONV) and any(spec.ops[j]['type'] in (ns.OP_CONV, ns.OP_DWCONV) and
                                                               o['out'] in (spec.ops[j]['in0'], spec.ops[j]['in1']) for j in idx):
                f[o['out']] = ('inner',)
        Y, E = xb.run_chain(spec, w, {i: gpu[i] for i in ins}, idx, f)
        r, at = xb.compare(gpu[t], Y[t], E[t])
        rows.append((name, t, producer[t], r))
        assert r <= 1.0, (f'launch {name!r}: op {producer[t]} ({[spec.ops[i].get("layer") or spec.ops[i]["type"] for i in idx]}) tensor {t}: '
                          f'error / E = {r:.3g} at element [b, y, x, c] = {at}: gpu {gpu[t][at]!r}, ref {Y[t][at]!r}, E {E[t][at]:.3g}')
    return names, rows, over


def _report(title, names, rows, over, t0):
    print(f'\n{title}: {len(names)} launches, {len(rows)} tensors checked, worst error / E = {max(r[3] for r in rows):.3f}, '
          f'worst over-estimate 2^{np.log2(max(over, 1)):.1f}, {time.time() - t0:.1f} s')
    for name, t, i, r in rows:
        print(f'    {r:6.3f}  op {i:3d} tensor {t:3d}  {name}')


def _layerwise_f16(spec, w, B, fuse=True, splitk=True, seed=0):
    """f16 -> (number of tensors checked, launch names)."""
    import torch
    from k210_yolo_framework_amd import engine
    frames = np.random.default_rng(seed).integers(0, 256, (B, *spec.in_hw, 3), dtype=np.uint8)
    with _switches({'YK_FUSE_DWPW': '1' if fuse else '0', 'YK_SPLITK': '1' if splitk else '0'}):
        plan = engine.Plan(spec, w, max_batch=B, precision='f16')
        plan.run_u8(torch.from_numpy(frames).cuda())
        torch.cuda.synchronize()
        gpu = {0: oracle.normalise_u8(frames)}
        for op in spec.ops:
            if op['type'] in (ns.OP_UPSAMPLE, ns.OP_CONCAT):
                continue
            try:
                gpu[op['out']] = plan.read_tensor(op['out'], B)
            except engine.YkError as e:
                if 'fused away' not in str(e):
                    raise
                # fused away: lives only in LDS / registers
        names = [l[0] for l in plan.launches()]
        plan.close()
    cp = spec.compile_plan(w)
    producer = {op['out']: i for i, op in enumerate(spec.ops)}
    checked, worst = 0, 0.0
    for i, op in enumerate(spec.ops):
        t = op['out']
        if t not in gpu or op['type'] in (ns.OP_UPSAMPLE, ns.OP_CONCAT):
            continue
        rows, inputs = [], {}

        def need(tid):
            if tid in gpu and tid != t:
                inputs[tid] = gpu[tid]
                return
            j = producer[tid]
            o = spec.ops[j]
            need(o['in0'])
            if o['in1'] >= 0:
                need(o['in1'])
            if j not in rows:
                rows.append(j)
        need(t)
        ref = oracle.net_forward_ex(cp, inputs, sorted(rows), [t], emulate_f16=True)[0]
        got = gpu[t]
        rms = float(np.sqrt((ref.astype(np.float64) ** 2).mean()))
        err = np.abs(got - ref)
        is_out = t in spec.outputs                  # network outputs are fp32: no fp16 rounding to flip
        bound = (1e-4 * np.abs(ref) + 1e-4 * rms) if is_out else (2.0 ** -9 * np.abs(ref) + 1e-3 * rms)
        bad = err > bound
        frac = 0.0 if is_out else float((got != ref).mean())
        assert not bad.any(), (f'op {i} {op.get("layer")} tensor {t} ({len(rows)} ops): {int(bad.sum())} elements beyond 1 ulp; '
                               f'max err {float(err.max()):.4g}, rms {rms:.4g}')
        assert frac < 0.02, f'op {i} {op.get("layer")}: {frac:.3%} of elements differ'
        worst = max(worst, float((err / np.maximum(bound, 1e-30)).max()))
        checked += 1
    return checked, names
