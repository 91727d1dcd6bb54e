#!/usr/bin/env python3
"""What contribution-based pruning costs and buys on the bench scene.

    python tools/contrib_prune_measure.py [--views 100] [--steps 100] [--threshold 0.01] [--no-grow]

One JSON line per measurement:
  * gs_render_contrib next to the fused forward of the same view, same process: device events around 20 calls after 3, on
    the bench scene (c3: 300 k Gaussians, 800 x 800) and on that scene grown to the reference schedule's cap by the
    trainer's own iterations 450 .. 1600 (bench.py's c3_grown_1m);
  * on the grown scene: the count, the step time (device events around --steps steps of the fused train step, densify off
    inside the timed loops so that neither holds an event) and the mean PSNR of the training views against their targets,
    before and after GaussianTrainer.pruneByContribution(cameras, threshold) over the training cameras, and the PSNR again
    after --steps further steps on the pruned model; the wall time of the prune event itself."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--no-grow", action="store_true")
    args = ap.parse_args()
    import torch
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.scenes import CONFIGS, GROW_ITERATIONS, make_config, perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel

    _, N, W, H, _ = CONFIGS["c3_300k_800"]
    params, cams, _ = make_config("c3_300k_800", n_views=args.views)
    V = len(cams)
    r = GaussianRenderer(4, W, H, (16, 16), False)
    gcams = [r._camera(c.worldViewTransform, c.projectionMatrix, c.cameraCenter, c.FoVx, c.FoVy, c.focalX, c.focalY) for c in cams]
    r.reserve(1_600_000, 48 << 20)
    tp = {k: torch.as_tensor(v, device=r.device) for k, v in perturb(params, 12345).items()}
    targets = [r.renderForward(tp, c).render.clone() for c in cams]
    del tp
    model = GaussModel(params, r.device, capacity=1_600_000)
    tr = GaussianTrainer(model, r, iterationCount=30000)
    tr.iteration = 450

    def events(body, n=20, warm=3):
        for _ in range(warm):
            body()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            body()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    def kernel_times(tag):
        p = model.getParams()
        maxW, sumW = torch.zeros(model.N, device=r.device), torch.zeros(model.N, device=r.device)
        fwd = events(lambda: r.renderForward(p, gcams[0], wantDepth=False))
        r.renderChecked(p, gcams[0], wantDepth=False)
        both = events(lambda: r.renderContrib(maxW, sumW))
        only_max = events(lambda: r.renderContrib(maxW, None))
        st = r.stats()
        print(json.dumps(dict(measure="render_contrib", scene=tag, N=model.N, M=int(st["M"]), forward_ms=round(fwd, 4),
                              contrib_ms=round(both, 4), contrib_max_only_ms=round(only_max, 4),
                              ratio=round(both / fwd, 3))), flush=True)

    def psnr():
        p = model.getParams()
        tot = 0.0
        for c, t in zip(cams, targets):
            mse = float(((r.renderChecked(p, c, wantDepth=False).render - t) ** 2).mean())
            tot += -10.0 * float(torch.log10(torch.tensor(max(mse, 1e-20))))
        return tot / V

    step_no = [0]

    def steps(n):
        for _ in range(n):
            v = step_no[0] % V
            tr.trainStep(gcams[v], targets[v], viewKey=v)
            step_no[0] += 1

    def step_time(n):
        dens, tr.densify = tr.densify, False
        steps(2 * V if n else 0)          # every view seen on this model: hints, cuts, target statistics
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        steps(n)
        b.record()
        torch.cuda.synchronize()
        tr.densify = dens
        return a.elapsed_time(b) / n

    kernel_times("c3_300k_800")
    if args.no_grow:
        return
    steps(GROW_ITERATIONS)
    r.sync()
    kernel_times("c3_grown_1m")
    before = dict(N=model.N, ms_per_step=round(step_time(args.steps), 4), psnr=round(psnr(), 3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = tr.pruneByContribution(cams, args.threshold)
    torch.cuda.synchronize()
    event_ms = (time.perf_counter() - t0) * 1e3
    after = dict(N=model.N, psnr_right_after=round(psnr(), 3), ms_per_step=round(step_time(args.steps), 4))
    after["psnr_after_steps"] = round(psnr(), 3)
    print(json.dumps(dict(measure="prune", scene="c3_grown_1m", threshold=args.threshold, views=V, stats=st,
                          event_wall_ms=round(event_ms, 1), before=before, after=after,
                          steps_between=args.steps + 2 * V)), flush=True)
    kernel_times("c3_grown_1m_pruned")


if __name__ == "__main__":
    main()
