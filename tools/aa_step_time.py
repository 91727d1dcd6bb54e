#!/usr/bin/env python3
"""Step time of the single-device fused train step with the anti-aliased mode off and on (GaussianRenderer.setAntialiased).

    python tools/aa_step_time.py [--configs c3_300k_800,c5_garden_2m] [--views 20] [--steps 200] [--warmup 2] [--rounds 2]

Per config, both modes train the same scene from the same start (a fresh model per run, densify off, every view visited
--warmup times before timing); the modes alternate --rounds times in one process.  One JSON line per run: ms per step over
--steps steps (device events around the whole loop), and the workload of a forward of view 0 in that mode from the start
parameters: the pair count M (gs_last_stats: the lists are built from the geometry alone, so the mode leaves it alone) and
the mean / total per-pixel contributor count nContrib (gs_copy_last_contrib: the blend's work, which the mode's alphas move)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3_300k_800,c5_garden_2m")
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    args = ap.parse_args()
    import torch
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.scenes import CONFIGS, make_config, perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    for config in args.configs.split(","):
        idx, N, W, H, _ = CONFIGS[config]
        params, cams, _ = make_config(config, n_views=args.views)
        r = GaussianRenderer(4, W, H, (16, 16), False)
        r.reserve(N, {0: 2 << 20, 1: 12 << 20, 2: 24 << 20}.get(idx, 96 << 20))
        tp = {k: torch.as_tensor(v, device=r.device) for k, v in perturb(params, 12345).items()}
        targets = [r.renderForward(tp, c).render.clone() for c in cams]
        del tp
        start = {k: torch.as_tensor(v, device=r.device) for k, v in params.items()}
        work = {}
        for on in (False, True):
            r.setAntialiased(on)
            r.renderForward(start, cams[0])
            nc = r.lastContrib().double()
            work[on] = dict(M=int(r.stats()["M"]), ncontrib_mean=round(float(nc.mean()), 3), ncontrib_sum=int(nc.sum()))
        del start
        V = len(cams)
        for _ in range(args.rounds):
            for on in (False, True):
                r.setAntialiased(on)
                model = GaussModel(params, r.device)
                tr = GaussianTrainer(model, r, iterationCount=30000, densify=False)
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
                print(json.dumps(dict(config=config, antialiased=on, steps=args.steps,
                                      ms_per_step=round(a.elapsed_time(b) / args.steps, 4), loss=float(tr._loss[0]),
                                      **work[on])), flush=True)
                del tr, model
        r.setAntialiased(False)
        r.close()
        del r, targets


if __name__ == "__main__":
    main()
