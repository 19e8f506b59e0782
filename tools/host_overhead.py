#!/usr/bin/env python3
"""Host-side cost of one forward call (ctypes marshalling + hipLaunchKernel), and CUDA-graph replay of the same call."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonic_flash_attention_amd import ops
dev = torch.device("cuda:0")
B, H, S, D = 2, 4, 128, 64          # BASELINE config C1 shape
q, k, v = (torch.randn(B, S, H, D, device=dev).to(torch.bfloat16).permute(0, 2, 1, 3) for _ in range(3))
out = torch.empty(B, S, H, D, device=dev, dtype=torch.bfloat16).permute(0, 2, 1, 3)
for _ in range(50):
    ops.fa3_forward(q, k, v, out=out)
torch.cuda.synchronize()
N = 3000
t = time.perf_counter()
for _ in range(N):
    ops.fa3_forward(q, k, v, out=out)
t_enq = (time.perf_counter() - t) / N
torch.cuda.synchronize()
t_all = (time.perf_counter() - t) / N
print(f"eager: enqueue {t_enq * 1e6:.1f} us/call, end-to-end {t_all * 1e6:.1f} us/call")
g = torch.cuda.CUDAGraph()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    ops.fa3_forward(q, k, v, out=out)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        for _ in range(10):
            ops.fa3_forward(q, k, v, out=out)
torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(N // 10):
    g.replay()
torch.cuda.synchronize()
print(f"graph (10 calls per replay): {(time.perf_counter() - t) / N * 1e6:.1f} us/call")
# one eager serving step over a paged cache: the append and the decode behind it (two launches), Hkv 2, 2 pages of 64 keys per sequence
kp, vp = (torch.randn(4, 64, 2, D, device=dev).to(torch.bfloat16).transpose(1, 2) for _ in range(2))
table = torch.tensor([[0, 1], [2, 3]], dtype=torch.int32, device=dev)
lens = torch.tensor([100, 128], dtype=torch.int32, device=dev)
q1, k1, v1 = (torch.randn(B, 1, h, D, device=dev).to(torch.bfloat16).permute(0, 2, 1, 3) for h in (H, 2, 2))
step = lambda: ops.fa3_decode(q1, kp, vp, cache_seqlens=lens, block_table=table, k_new=k1, v_new=v1)
for _ in range(50):
    step()
torch.cuda.synchronize()
t = time.perf_counter()
for _ in range(N):
    step()
t_enq = (time.perf_counter() - t) / N
torch.cuda.synchronize()
print(f"paged decode step (k_new / v_new): enqueue {t_enq * 1e6:.1f} us/step, end-to-end {(time.perf_counter() - t) / N * 1e6:.1f} us/step")
