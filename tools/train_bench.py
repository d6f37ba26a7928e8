#!/usr/bin/env python3
"""Wall time of the fused training step alone (bench.py's train_step leg): python tools/train_bench.py [B=rows] [steps] [lib ...]
Several libraries (paths under cadm_amd/, or absolute) are timed interleaved, three rounds."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from cadm_amd import _lib

args = sys.argv[1:]
B = int(args.pop(0)[2:]) if args and args[0].startswith("B=") else 256
steps = int(args[0]) if args else 300
libs = args[1:] or [None]
for rnd in range(3 if len(libs) > 1 else 1):
    for path in libs:
        lib = _lib.load_dev(os.path.join(ROOT, "cadm_amd", path)) if path else None
        r = bench.train_step_bench("cuda:0", lib, steps=steps, warmup=20, B=B)
        print(path or "product", json.dumps(r))
