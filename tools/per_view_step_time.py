#!/usr/bin/env python3
"""Step time of the single-device fused train step without a per-view correction and with each of them: camera pose
refinement, exposure compensation, the bilateral grid (GaussianTrainer(pose_opt=True) / (exposure_opt=True) /
(bilateral_grid=True)).

    python tools/per_view_step_time.py [--config c3_300k_800] [--steps 200] [--warmup 2] [--rounds 3] [--modes off,pose,exposure,grid]

Every mode trains the same scene from the same start (a fresh model per run, densify off, every view visited --warmup times
before timing); the modes alternate --rounds times in one process.  One JSON line per run: ms per step over --steps steps
(device events around the whole loop)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3_300k_800")
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="off,pose,exposure,grid")
    args = ap.parse_args()
    import torch
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.scenes import CONFIGS, make_config, perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    idx, N, W, H, _ = CONFIGS[args.config]
    params, cams, _ = make_config(args.config, n_views=args.views)
    r = GaussianRenderer(4, W, H, (16, 16), False)
    r.reserve(N, {0: 2 << 20, 1: 12 << 20, 2: 24 << 20}.get(idx, 96 << 20))
    tp = {k: torch.as_tensor(v, device=r.device) for k, v in perturb(params, 12345).items()}
    targets = [r.renderForward(tp, c).render.clone() for c in cams]
    del tp
    V = len(cams)
    kws = {"off": {}, "pose": dict(pose_opt=True, n_views=V), "exposure": dict(exposure_opt=True, n_views=V),
           "grid": dict(bilateral_grid=True, n_views=V)}
    for _ in range(args.rounds):
        for mode in args.modes.split(","):
            model = GaussModel(params, r.device)
            tr = GaussianTrainer(model, r, iterationCount=30000, densify=False, **kws[mode])
            tr.iteration = 1
            for i in range(args.warmup * V):
                tr.trainStep(cams[i % V], targets[i % V], viewKey=i % V)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(args.steps):
                v = (args.warmup * V + i) % V
                tr.trainStep(cams[v], targets[v], viewKey=v)
            b.record()
            torch.cuda.synchronize()
            print(json.dumps(dict(config=args.config, mode=mode, steps=args.steps,
                                  ms_per_step=round(a.elapsed_time(b) / args.steps, 4), loss=float(tr._loss[0]))), flush=True)
            del tr, model


if __name__ == "__main__":
    main()
