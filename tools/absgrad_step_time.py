#!/usr/bin/env python3
"""Step time of the single-device fused train step with AbsGS densification off and on (GaussianTrainer(absgrad=...)), and the
Gaussian count each criterion leaves behind the first densify events.

    python tools/absgrad_step_time.py [--config c3_300k_800] [--views 20] [--steps 200] [--warmup 2] [--rounds 3]
                                      [--events 3] [--event-every 100]

Timing.  Both modes train the bench scene from the same start (a fresh model per run, densify ON so that the statistic is
accumulated in both -- |grad xyz| in the projection backward, or hypot(W/2 Ax, H/2 Ay) behind the blend backward --, no densify
event inside the window, every view visited --warmup times before timing); the modes alternate --rounds times in one process.
One JSON line per run: ms per step over --steps steps (device events around the whole loop, ended by a synchronise).

Counts.  Then each mode trains --events x --event-every steps with a densify event every --event-every steps (from step 1; the
reference's thresholds, the mode's own gradientThreshold) and prints N and the event's action counts behind each event."""
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
    ap.add_argument("--events", type=int, default=3)
    ap.add_argument("--event-every", type=int, default=100)
    args = ap.parse_args()
    import torch
    from gaussiansplattingmlx_amd.absgrad import AbsGradConfig
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.scenes import CONFIGS, make_config, perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    if not torch.cuda.is_available():
        raise SystemExit("absgrad_step_time: no GPU (a timing taken anywhere else says nothing)")
    config = args.config
    idx, N, W, H, _ = CONFIGS[config]
    params, cams, _ = make_config(config, n_views=args.views)
    r = GaussianRenderer(4, W, H, (16, 16), False)
    r.reserve(N, {0: 2 << 20, 1: 12 << 20, 2: 24 << 20}.get(idx, 96 << 20))
    tp = {k: torch.as_tensor(v, device=r.device) for k, v in perturb(params, 12345).items()}
    targets = [r.renderForward(tp, c).render.clone() for c in cams]
    del tp
    V = len(cams)

    def trainer(on, densify_from):
        r.setAbsgrad(False)           # (a trainer turns the setting on and leaves it on)
        model = GaussModel(params, r.device)
        tr = GaussianTrainer(model, r, iterationCount=30000, absgrad=AbsGradConfig() if on else None)
        tr.densifyFromIter = densify_from
        tr.iteration = 1
        return tr, model

    for _ in range(args.rounds):
        for on in (False, True):
            tr, model = trainer(on, 1 << 30)
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
            print(json.dumps(dict(config=config, absgrad=on, steps=args.steps, N=model.N,
                                  ms_per_step=round(a.elapsed_time(b) / args.steps, 4), loss=float(tr._loss[0]))), flush=True)
            del tr, model
    for on in (False, True):
        tr, model = trainer(on, 1)
        tr.split_and_prune_per_iteration = args.event_every
        seen = None
        for i in range(args.events * args.event_every + 1):
            tr.trainStep(cams[i % V], targets[i % V], viewKey=i % V)
            if tr.lastDensifyStats is not None and tr.lastDensifyStats is not seen:
                seen = tr.lastDensifyStats
                print(json.dumps(dict(config=config, absgrad=on, threshold=tr.gradientThreshold, after_step=i + 1, N=model.N,
                                      event=seen)), flush=True)
        del tr, model
    r.setAbsgrad(False)
    r.close()


if __name__ == "__main__":
    main()
