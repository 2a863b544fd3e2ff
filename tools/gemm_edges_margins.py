"""Folds the `gemm-margins path output ratio case` lines that tests/test_gpu_gemm_edges.py prints into the table of
profiles/gemm_edges_margins.txt: the largest err / bound per path and the case that gave it.
    python -m pytest -m gpu -s tests/test_gpu_gemm_edges.py > raw.txt && python tools/gemm_edges_margins.py raw.txt"""
import re
import sys

worst = {}
for line in open(sys.argv[1]):
    m = re.search(r'gemm-margins (\S+) (\S+) (\S+) (.*?)(?: PASSED| FAILED)?$', line.rstrip())
    if m:
        path, out, ratio, case = m.groups()
        if (path, out) not in worst or float(ratio) > worst[(path, out)][0]:
            worst[(path, out)] = (float(ratio), case.strip())
print('yk_gemm_f32 and yk_conv3x3_* on normal data against float64 (tests/test_gpu_gemm_edges.py), one MI355X: the largest err / bound per path.')
print('bound per element: gamma(K + 4) (|alpha| |A| |B| + |beta| |C0|), gamma(n) = n u / (1 - n u), u = 2^-24, K the length of the reduction.')
print('GEMM paths: layout / loader / tile epilogue(s) / finishing pass.  1.0 would be a failure.\n')
print(f'{"path":32}{"output":8}{"err/bound":>10}  case')
for (path, out), (r, case) in sorted(worst.items()):
    print(f'{path:32}{out:8}{r:10.2e}  {case}')
