"""One MS-TCT teacher window (T = 256, D = 2048, ivt head) under rocprofv3: warm-up, then 20 eager windows and 20 hipGraph replays.
cd /tmp && rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o mstct -- python3 <repo>/tools/mstct_infer_prof.py"""
import os, sys, types, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from computervision_codes_amd import shapes, synth
from computervision_codes_amd.temporal_mstct import VideoNas
from computervision_codes_amd.graph import GraphedForward
args = types.SimpleNamespace(loss_type="ivt")
inter = [256, 384, 576, 864]
m = VideoNas(args, inter, 2, 8, 8, 2048, 512).eval()
m.load_state_dict(synth.fill_from_shapes(shapes.mstct_shapes(2048, inter, 2, 8, 512, "ivt"), seed=3))
x = synth.synthetic_features(256, 2048, seed=3).cuda()
for _ in range(3): m.forward_btd(x)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(20): m.forward_btd(x)
torch.cuda.synchronize(); print("eager window ms", round((time.perf_counter() - t0) / 20 * 1e3, 4))
g = GraphedForward(lambda xx: m.forward_btd(xx), [x])
for _ in range(3): g(x)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(20): g(x)
torch.cuda.synchronize(); print("graph window ms", round((time.perf_counter() - t0) / 20 * 1e3, 4))
