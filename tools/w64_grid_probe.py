"""Launch the 64-rows-per-wave forward at given shapes, with FA_W64_PERSIST=1 and then =0, on random data: run under `rocprofv3 --kernel-trace`, the trace's Grid_Size_X
of the two dispatches per shape says whether the first was a persistent launch (one workgroup per CU walking the blocks) and the second one workgroup per block
(launch_fwd_w64_t decides from the shape, the mask and the knob alone).  tests/test_softmax_profiles_gpu.py runs it that way.
usage: w64_grid_probe.py dtype B,Sq,Sk,H,Hk,D,causal [...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "flash-attention_amd"))
import torch
from flash_attn_amd import backend as be

dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[sys.argv[1]]
os.environ["FA_FWD_NW"] = "64"
for shape in sys.argv[2:]:
    B, Sq, Sk, H, Hk, D, causal = (int(x) for x in shape.split(","))
    q = torch.randn(B, Sq, H, D, device="cuda", dtype=dtype)
    k = torch.randn(B, Sk, Hk, D, device="cuda", dtype=dtype)
    v = torch.randn_like(k)
    for persist in (1, 0):
        os.environ["FA_W64_PERSIST"] = str(persist)
        be.reload_knobs()
        be.fwd(q, k, v, None, None, 0.0, D ** -0.5, bool(causal), -1, -1, 0.0, False, None)
        s = be.last_schedule()
        assert s["fwd_kernel"] == 3, s
        print("%s persist=%d %s" % (shape, persist, s["name"]))
torch.cuda.synchronize()
