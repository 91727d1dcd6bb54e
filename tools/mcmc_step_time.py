#!/usr/bin/env python3
"""Cost of the MCMC strategy (GaussianTrainer(strategy="mcmc"); include/gsplat.h gs_set_mcmc).

    python tools/mcmc_step_time.py [--config c3_300k_800] [--views 20] [--steps 200] [--warmup 2] [--rounds 2]
                                   [--event-n 300000,1000000] [--events 5]

Step: the single-device fused train step of --config with the strategy off (densify off), on at the same N (cap_max = N, no
event in the timed window: the regularisers and the noise in the fused backward + Adam), and on with zero regularisers and
zero noise_lr (the same kernels and instructions, but the trajectory of the default step: the kernels' own cost, apart from
what the strategy does to the scene), alternating --rounds times in one process; ms per step over --steps steps (device events
around the loop) and the pair count M of the last forward (the workload the scene has become).  Event: relocation + growth (gs_mcmc_relocate,
gs_mcmc_grow) on a random model (K = 25) of each --event-n Gaussians, ~10 % of them below min_opacity, host
wall time of the two calls (each waits for its counts) after a device drain, --events times from a fresh copy of the model.
One JSON line per run."""
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
    ap.add_argument("--config", default="c3_300k_800")
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--event-n", default="300000,1000000")
    ap.add_argument("--events", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.scenes import CONFIGS, make_config, perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel

    idx, N, W, H, _ = CONFIGS[args.config]
    params, cams, _ = make_config(args.config, n_views=args.views)
    N = int(params["xyz"].shape[0])
    r = GaussianRenderer(4, W, H, (16, 16), False)
    r.reserve(N, {0: 2 << 20, 1: 12 << 20, 2: 24 << 20}.get(idx, 96 << 20))
    tp = {k: torch.as_tensor(v, device=r.device) for k, v in perturb(params, 12345).items()}
    targets = [r.renderForward(tp, c).render.clone() for c in cams]
    del tp
    V = len(cams)
    for _ in range(args.rounds):
        for on in ("off", "on", "on_zero_terms"):
            model = GaussModel(params, r.device)
            zero = dict(noise_lr=0.0, opacity_reg=0.0, scale_reg=0.0) if on == "on_zero_terms" else {}
            kw = dict(strategy="mcmc", mcmc=MCMCConfig(cap_max=N, refine_start=10 ** 9, **zero)) if on != "off" else dict(densify=False)
            tr = GaussianTrainer(model, r, iterationCount=30000, **kw)
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
            print(json.dumps(dict(kind="step", config=args.config, N=N, mcmc=on, steps=args.steps,
                                  ms_per_step=round(a.elapsed_time(b) / args.steps, 4), loss=float(tr._loss[0]),
                                  M=int(r.stats()["M"]))), flush=True)
            del tr, model
    del targets
    for n in (int(x) for x in args.event_n.split(",") if x):
        rng = np.random.default_rng(1)
        p = dict(xyz=rng.uniform(-1, 1, (n, 3)), features_dc=rng.normal(0, 1, (n, 1, 3)),
                 features_rest=rng.normal(0, 0.01, (n, 24, 3)), scales=rng.normal(-4, 0.5, (n, 3)),
                 rotation=rng.normal(0, 1, (n, 4)), opacity=rng.normal(0.0, 2.0, n))
        p = {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}
        p["opacity"][rng.random(n) < 0.1] = np.float32(-8.0)            # ~10 % dead (sigmoid(-8) = 3e-4 < 0.005)
        cfg = MCMCConfig(cap_max=int(n * 1.05) + 1)
        times = []
        for e in range(args.events + 1):
            model = GaussModel(p, r.device)
            model.restride(cfg.cap_max)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = r.mcmcRelocate(model.getParams(), model.arena, model.m, model.v, cfg.params(600 + e, 1))
            t1 = time.perf_counter()
            n1 = r.mcmcGrow(model.getParams(), model.stride, model.arena, model.m, model.v, cfg.params(600 + e, 1))
            t2 = time.perf_counter()
            if e > 0:         # (the first event pays for the scratch allocation)
                times.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
            del model
        rel = sorted(t[0] for t in times)
        grw = sorted(t[1] for t in times)
        print(json.dumps(dict(kind="event", N=n, events=len(times), dead=st["dead"], relocated=st["relocated"], N_after=n1,
                              relocate_ms_median=round(rel[len(rel) // 2], 4), grow_ms_median=round(grw[len(grw) // 2], 4),
                              event_ms_median=round(sorted(a + b for a, b in times)[len(times) // 2], 4))), flush=True)
    r.close()


if __name__ == "__main__":
    main()
