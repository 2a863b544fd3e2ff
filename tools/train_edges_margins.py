"""Folds the lines tests/test_gpu_train_edges.py appends to $YK_TRAIN_EDGES_MARGINS (`path output ratio case`) into the table of
profiles/train_edges_margins.txt: the largest err / bound per dispatch path and per output, and the case that gave it.
    YK_TRAIN_EDGES_MARGINS=raw.txt python -m pytest -m gpu tests/test_gpu_train_edges.py && python tools/train_edges_margins.py raw.txt"""
import sys

worst = {}
for line in open(sys.argv[1]):
    path, out, ratio, case = line.split(None, 3)
    if (path, out) not in worst or float(ratio) > worst[(path, out)][0]:
        worst[(path, out)] = (float(ratio), case.strip())
print('yk_bn_train_fwd_f32 + yk_bn_train_bwd_f32 against numpy float64 (tests/test_gpu_train_edges.py), one MI355X:')
print('largest err / bound per path of yk_bn_train_bwd_f32 and per output; bounds: y 2e-5 max|pre|; dbeta, dgamma 2e-4 sum|terms| + kink')
print('slack per column; dz 2e-4 max|dz| + kink widening per element.  1.0 would be a failure.\n')
print(f'{"path":8}{"output":8}{"err/bound":>10}  case (M, C, act, alpha)')
for (path, out), (r, case) in sorted(worst.items()):
    print(f'{path:8}{out:8}{r:10.2e}  {case}')
