"""Per-op times of resnet18 against resnet18_fp8 at B = 256 on cuda:0
(InferenceEngine.profile: hipEvent pairs around every op of an eager forward),
the two engines' profiled forwards interleaved, the minimum of 5 per op, and
the single-forward sums: the numbers of profiles/resnet18_fp8.txt.
python tools/profile_resnet18_fp8.py [out.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from dmlc.models import state_dict_f32
from dmlc.models.calibrated import calibrated, mixed_images
from dmlc.runtime import InferenceEngine

B = 256
sd = state_dict_f32(calibrated("resnet18", seed=11))
x = mixed_images(B, seed=12).cuda()
engs = {a: InferenceEngine(a, sd, max_batch=B) for a in ("resnet18", "resnet18_fp8")}
for e in engs.values():
    for _ in range(3):
        e.profile(x)
runs = {a: [] for a in engs}
for _ in range(5):
    for a, e in engs.items():
        runs[a].append(dict(e.profile(x)))
best = {a: {k: min(r[k] for r in rs) for k in rs[0]} for a, rs in runs.items()}
lines = [f"InferenceEngine.profile, B = {B}, one MI355X, one session; the engines' forwards interleaved,",
         "minimum of 5 per op (us); sum = the smallest single forward's sum of its ops", "",
         f"{'op':28s} {'resnet18':>10s} {'resnet18_fp8':>13s}"]
for k in best["resnet18"]:
    lines.append(f"{k:28s} {best['resnet18'][k] * 1e3:10.1f} {best['resnet18_fp8'].get(k, float('nan')) * 1e3:13.1f}")
sums = {a: min(sum(r.values()) for r in rs) * 1e3 for a, rs in runs.items()}
lines.append(f"{'sum of one forward':28s} {sums['resnet18']:10.1f} {sums['resnet18_fp8']:13.1f}")
text = "\n".join(lines) + "\n"
print(text)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(text)
