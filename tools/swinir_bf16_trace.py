"""The 5D SwinIR inference on bf16 storage alone (8 x 256 x 256, 7 calls), for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o sw -- python tools/swinir_bf16_trace.py
    python tools/kstats.py OUT/.../sw_kernel_trace.csv 7 30 --all
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from basicsr.archs import build_network
from dcpt_amd.keyed_init import fill_module_

cfg = dict(embed_dim=180, depths=[6] * 6, num_heads=[6] * 6, mlp_ratio=2.0, window_size=8, upscale=1)
dev = torch.device("cuda:0")
net = fill_module_(build_network(dict(type="SwinIR", act_dtype="bf16", **cfg))).to(dev).eval()
x = torch.rand((8, 3, 256, 256), device=dev)
with torch.no_grad():
    for _ in range(7):
        net(x)
torch.cuda.synchronize()
print("done")
