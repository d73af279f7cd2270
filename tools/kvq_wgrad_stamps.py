"""Diagnostic: phase timeline of two workgroups of the deferred K / V / Q / f_W weight-gradient launch INSIDE the C2 training step
(s_memtime per wave; fp32 kernel, PS_GEMM_STAMP=5): split 1, tile (0, 0) of the listed K member and of the plain Q member.
    python tools/kvq_wgrad_stamps.py [PS_KVQ_SPLIT value]      (on the GPU box; diagnostic library)"""
import argparse, ctypes, os, sys
os.environ['PS_DIAG_LIB'] = '1'      # stamps exist in the diagnostic build only (python -m prodsearch_amd.build --diag)
os.environ['PS_GEMM_STAMP'] = '5'
if len(sys.argv) > 1:
    os.environ['PS_KVQ_SPLIT'] = sys.argv[1]
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from prodsearch_amd import _lib

a = argparse.Namespace(workload='c2', encoder='pvc', dropout=0.1, row_sparse=False, sharded=False)
wl = bench.TemWorkload(a, 'c2', 0, torch.device('cuda', 0))
wl.model.train()
raw = ctypes.CDLL(_lib.lib_path())


def step(i):
    loss = wl.forward(i)
    wl.model.zero_grad()
    loss.backward()
    wl.optim.step()


for i in range(8):
    step(i)
torch.cuda.synchronize()
buf = torch.zeros(512, dtype=torch.int64, device='cuda')
raw.ps_debug_set_stamp_buffer(ctypes.c_void_p(buf.data_ptr()))
step(9)
torch.cuda.synchronize()
raw.ps_debug_set_stamp_buffer(ctypes.c_void_p(0))
names = {0: 'start', 1: 'list length known', 2: 'row indices in LDS', 3: 'first slabs requested', 4: 'first slab in LDS', 31: 'epilogue issued'}
for s in range(16):
    names[5 + s] = 'slab %d done' % s
for off, who in ((256, 'listed K member'), (384, 'plain Q member')):
    t = buf.cpu()[off:off + 128].view(4, 32)
    live = [w for w in range(4) if int(t[w, 0])]
    t0 = min(int(t[w, 0]) for w in live) if live else 0
    print('%s, split 1, tile (0, 0)' % who)
    print('%-30s' % 'phase' + ''.join('   wave%d' % w for w in range(4)) + '   (s_memtime: shader-clock cycles since the first wave started)')
    for i in range(32):
        if i in names and any(int(t[w, i]) for w in range(4)):
            print('%-30s' % names[i] + ''.join('%8d' % (int(t[w, i]) - t0 if int(t[w, i]) else -1) for w in range(4)))
