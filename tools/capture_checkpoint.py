#!/usr/bin/env python3
"""Store the reference's trained checkpoint (saved_models/narde_model_final.pt,
a DecomposedDQN state dict, 2.8 MB of float32) as test fixtures (test
infrastructure): tests/golden/checkpoint_<k>.npz, each below 1 MiB.  Every
tensor is kept bit for bit under its state-dict key; one too large for a
file is cut along its rows into pieces named <key>@<first row>
(tests/test_dqn_cpu.py puts them together again).
Usage: python tools/capture_checkpoint.py <reference>/saved_models/narde_model_final.pt"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PART_BYTES = 960 * 1024


def main():
    sd = torch.load(sys.argv[1], weights_only=True, map_location="cpu")
    pieces = []
    for key, t in sd.items():
        a = t.numpy()
        n = max(1, -(-a.nbytes // PART_BYTES))
        rows = -(-a.shape[0] // n)
        for r in range(0, a.shape[0], rows):
            pieces.append((key if n == 1 else f"{key}@{r}", a[r:r + rows]))
    parts, size = [{}], 0
    for name, a in pieces:
        if size + a.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][name] = a
        size += a.nbytes
    for k, part in enumerate(parts):
        path = os.path.join(HERE, "..", "tests", "golden", f"checkpoint_{k}.npz")
        np.savez_compressed(path, **part)
        print(os.path.normpath(path), os.path.getsize(path), sorted(part))


if __name__ == "__main__":
    main()
