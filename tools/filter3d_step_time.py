#!/usr/bin/env python3
"""Step time of the single-device fused train step in the anti-aliased mode with the 3-D smoothing filter off and on
(GaussianTrainer(filter_3d=True)), and the time of the filter-width kernel on its own.

    python tools/filter3d_step_time.py [--configs c3_300k_800,c5_garden_2m] [--views 20] [--steps 200] [--warmup 2] [--rounds 2]
                                       [--width 300000x100,300000x300,1000000x100,1000000x300]

Per config, both modes train the same scene from the same start on an anti-aliased renderer (a fresh model per run, densify
off, every view visited --warmup times before timing); the modes alternate --rounds times in one process.  The filter's
cameras are the run's training views; the filter is recomputed every 100 steps (the trainer's default), inside the timed loop.
One JSON line per run: ms per step over --steps steps (device events around the whole loop), and the workload of a forward of
view 0 in that mode from the start parameters: the pair count M (gs_last_stats; s_eff >= s, so radii and pairs can grow) and
the mean / total per-pixel contributor count nContrib (gs_copy_last_contrib).

--width: gs_compute_filter3d alone at N Gaussians x V cameras (positions of a cube, cameras on a ring): device events around
20 calls after 3, one JSON line each with us per call and its share of a 100-step window at the given ms per step."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def width_times(spec, window_ms_per_step):
    import numpy as np
    import torch
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    r = GaussianRenderer(4, 64, 64, (16, 16), False)
    for item in spec.split(","):
        N, V = (int(x) for x in item.split("x"))
        rng = np.random.default_rng(5)
        cams = [Camera(800, 800, 900.0, 900.0, look_at_c2w([4.5 * np.cos(a), 4.5 * np.sin(a), 1.0 + np.sin(3 * a)]))
                for a in np.linspace(0, 2 * np.pi, V, endpoint=False)]
        r.setFilterCameras(cams)
        xyz = torch.as_tensor(rng.uniform(-1.5, 1.5, (N, 3)).astype(np.float32), device=r.device)
        out = torch.empty(N, device=r.device)
        for _ in range(3):
            r.computeFilter3D(xyz, out=out)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            r.computeFilter3D(xyz, out=out)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) / 20 * 1e3
        print(json.dumps(dict(width_kernel=item, us_per_call=round(us, 2), pairs_per_ns=round(N * V / (us * 1e3), 2),
                              share_of_100_steps=round(us * 1e-3 / (100 * window_ms_per_step), 6),
                              window_ms_per_step=window_ms_per_step, mean_width=float(out.mean()))), flush=True)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3_300k_800,c5_garden_2m")
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--width", default="")
    ap.add_argument("--window-ms-per-step", type=float, default=0.75)
    args = ap.parse_args()
    import torch
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.scenes import CONFIGS, make_config, perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    for config in [c for c in args.configs.split(",") if c]:
        idx, N, W, H, _ = CONFIGS[config]
        params, cams, _ = make_config(config, n_views=args.views)
        r = GaussianRenderer(4, W, H, (16, 16), False, antialiased=True)
        r.reserve(N, {0: 2 << 20, 1: 12 << 20, 2: 24 << 20}.get(idx, 96 << 20))
        tp = {k: torch.as_tensor(v, device=r.device) for k, v in perturb(params, 12345).items()}
        targets = [r.renderForward(tp, c).render.clone() for c in cams]
        del tp
        start = {k: torch.as_tensor(v, device=r.device) for k, v in params.items()}
        r.setFilterCameras(cams)
        filt = r.computeFilter3D(start["xyz"])
        work = {}
        for on in (False, True):
            r.setFilter3D(filt if on else None)
            r.renderForward(start, cams[0])
            nc = r.lastContrib().double()
            work[on] = dict(M=int(r.stats()["M"]), ncontrib_mean=round(float(nc.mean()), 3), ncontrib_sum=int(nc.sum()))
        r.setFilter3D(None)
        width = dict(mean=float(filt.mean()), min=float(filt.min()), max=float(filt.max()))
        del start, filt
        V = len(cams)
        for _ in range(args.rounds):
            for on in (False, True):
                model = GaussModel(params, r.device)
                kw = dict(filter_3d=True, filter_cameras=cams) if on else {}
                tr = GaussianTrainer(model, r, iterationCount=30000, densify=False, **kw)
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
                print(json.dumps(dict(config=config, antialiased=True, filter_3d=on, steps=args.steps,
                                      ms_per_step=round(a.elapsed_time(b) / args.steps, 4), loss=float(tr._loss[0]),
                                      filter_width=width, **work[on])), flush=True)
                del tr, model
        r.close()
        del r, targets
    if args.width:
        width_times(args.width, args.window_ms_per_step)


if __name__ == "__main__":
    main()
