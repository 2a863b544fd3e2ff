"""Dev probe: is the training step host-bound?  Times eager steps vs a HIP-graph replay of the same launches."""
import sys, time
sys.path.insert(0, '.')
import torch
from bench import _train_setup
tr, x, y = _train_setup(16, 0, 1, 0)
for _ in range(3):
    tr.step(x, y)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(10):
    tr.step(x, y)
torch.cuda.synchronize()
print('eager ms/step', (time.perf_counter() - t0) / 10 * 1e3)
def body():
    r = tr.loss_and_grads(x, y)
    tr._ck('yk_adam_f32', tr.n_params, tr.P, tr.G, tr.m, tr.v, tr.lr, tr.decay, tr.iterations, 0.9, 0.999, 1e-7, 1.0)
    return r
s = torch.cuda.Stream()
s.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(s):
    body()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r = body()
torch.cuda.synchronize()
for _ in range(3):
    g.replay()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(10):
    g.replay()
torch.cuda.synchronize()
print('graph ms/step', (time.perf_counter() - t0) / 10 * 1e3)
