#!/usr/bin/env python3
"""Step time of the single-device fused train step with sparse Adam off and on (GaussianTrainer(sparse_adam=...)), the stage
time of the fused projection backward + Adam in both modes, and the share of the model the views see.

    python tools/sparse_adam_step_time.py [--config c3_300k_800] [--views 20] [--steps 200] [--warmup 2] [--rounds 3]
                                          [--profile-steps 40] [--eye-scale 1.0] [--unfused]

Both modes train the bench scene from the same start (a fresh model per run, densify off so that the count stays put, every view
visited --warmup times before timing); the modes alternate --rounds times in one process.  One JSON line per run: ms per step
over --steps steps (device events around the whole loop, ended by a synchronise), then -- over --profile-steps further steps
with the library's stage events on -- the mean gs_profile time of the projection forward (which holds the mask kernel) and of
the fused projection backward + Adam (without --unfused; the plain projection backward with it), and the mean visible share
of those steps' views.

--unfused: the trainer's fuse_adam=False step (backward into a gradient arena, then gs_adam_step or, with sparse Adam on,
gs_adam_step_visible); the `adam` stage time of those kernels is printed as well.

--eye-scale s: every camera's position is pulled towards the centre of the model by the factor s (its orientation kept), so
that a view sees a part of the model only; 1.0 leaves the bench views as they are.  The visible share is printed with each run.
"""
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
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=40)
    ap.add_argument("--eye-scale", type=float, default=1.0)
    ap.add_argument("--unfused", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from gaussiansplattingmlx_amd.camera import Camera
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.scenes import CONFIGS, make_config, perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    if not torch.cuda.is_available():
        raise SystemExit("sparse_adam_step_time: no GPU (a timing taken anywhere else says nothing)")
    config = args.config
    idx, N, W, H, _ = CONFIGS[config]
    params, cams, _ = make_config(config, n_views=args.views)
    if args.eye_scale != 1.0:
        centre = params["xyz"].astype(np.float64).mean(axis=0)
        moved = []
        for c in cams:
            c2w = np.array(c.c2w, np.float64)
            c2w[:3, 3] = centre + args.eye_scale * (c2w[:3, 3] - centre)
            moved.append(Camera(W, H, c.focalX, c.focalY, c2w))
        cams = moved
    r = GaussianRenderer(4, W, H, (16, 16), False)
    r.reserve(N, {0: 2 << 20, 1: 12 << 20, 2: 24 << 20}.get(idx, 96 << 20))
    tp = {k: torch.as_tensor(v, device=r.device) for k, v in perturb(params, 12345).items()}
    targets = [r.renderForward(tp, c).render.clone() for c in cams]
    del tp
    V = len(cams)

    for _ in range(args.rounds):
        for on in (False, True):
            model = GaussModel(params, r.device)
            tr = GaussianTrainer(model, r, iterationCount=30000, densify=False, sparse_adam=on, fuse_adam=not args.unfused)
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
            ms = a.elapsed_time(b) / args.steps
            # the stages, and what the views saw, over a few more steps
            r.profile(("proj_fwd", "proj_bwd", "adam"))
            r.profileRead()
            visible = 0
            for i in range(args.profile_steps):
                v = i % V
                tr.trainStep(cams[v], targets[v], viewKey=v)
                r.sync()
                visible += r.stats()["N_visible"]
            st = r.profileRead()
            r.profile(False)
            n = max(args.profile_steps, 1)
            print(json.dumps(dict(config=config, eye_scale=args.eye_scale, fuse_adam=not args.unfused, sparse_adam=on,
                                  steps=args.steps, N=model.N,
                                  ms_per_step=round(ms, 4), visible_share=round(visible / (n * model.N), 4),
                                  proj_fwd_ms=round(st["proj_fwd"][0] / max(st["proj_fwd"][1], 1), 4),
                                  proj_bwd_adam_ms=round(st["proj_bwd"][0] / max(st["proj_bwd"][1], 1), 4),
                                  adam_ms=round(st["adam"][0] / max(st["adam"][1], 1), 4),
                                  loss=float(tr._loss[0]))), flush=True)
            del tr, model
    r.close()


if __name__ == "__main__":
    main()
