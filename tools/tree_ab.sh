#!/bin/bash
# Same-box A-B-A-B of two source trees (the tree itself and a copy of an older one under ab_old/, each with its own built library):
#   bash tools/tree_ab.sh [rows] [T] [rounds]            -> steps/s of `tools/option_ab.py`-style timing per tree and round (sampling)
#   bash tools/tree_ab.sh [rows] [T] [rounds] train      -> ms per eager training step (forward + backward, FlatAdam, zero_grad; device-side
#                                                           draws) per tree and round, five repeats each and their spread
ROWS=${1:-65536}; T=${2:-50}; N=${3:-2}; MODE=${4:-sample}
for r in $(seq 1 $N); do
  for tree in ab_old .; do
    if [ "$MODE" = train ]; then
    (cd $tree && python3 - "$ROWS" "$T" "$tree" <<'PY'
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
import torch, bench
from diffsg_amd.train import FlatAdam
B, T, tag = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
dev = torch.device("cuda:0")
ddpm = bench.build_model(dev, T)
ddpm.device_draws = 1
opt = FlatAdam(ddpm, lr=1e-4)
cfg = ddpm.model.cfg
g = torch.Generator().manual_seed(B)
y = (torch.rand(B, cfg["input_dim"], generator=g) * 0.25).to(dev)
cond = torch.rand(B, cfg["cond_dim"], generator=g).to(dev)
def steps(n):
    for _ in range(n):
        loss = ddpm(y, cond); loss.backward(); opt.step(); opt.zero_grad()
    torch.cuda.synchronize()
steps(20)
n = 40 if B >= 8192 else 200
ms = []
for _ in range(5):
    t0 = time.perf_counter(); steps(n); ms.append((time.perf_counter() - t0) / n * 1e3)
print(f"{tag:7s} train {B} rows: " + " ".join(f"{v:.4f}" for v in ms) + f" ms/step  (min {min(ms):.4f}, spread {(max(ms) - min(ms)) / min(ms) * 100:.1f} %)", flush=True)
PY
    ) || exit 1      # a tree that fails ends the comparison: nothing more is started on the card
    else
    (cd $tree && python3 - "$ROWS" "$T" "$tree" <<'PY'
import os, sys, time
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests", "golden"))
import torch, bench
B, T, tag = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
dev = torch.device("cuda:0")
ddpm = bench.build_model(dev, T)
cond = torch.rand(B, 80, device=dev)
for _ in range(3): ddpm.sample(cond, 1.0, seed=1)
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(4): y = ddpm.sample(cond, 1.0, seed=1)
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 4 / T
ddpm.sample(cond, 1.0, seed=1, profile=True); torch.cuda.synchronize()
ops = {r[0][:14]: round(r[3] / T * 1e3, 1) for r in ddpm.op_profile() if r[3] / T > 8e-3}
print(f"{tag:7s} {dt*1e3:.4f} ms/step = {1/dt:.1f} steps/s  {ops}", flush=True)
PY
    ) || exit 1      # a tree that fails ends the comparison: nothing more is started on the card
    fi
  done
done
