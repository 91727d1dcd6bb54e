#!/usr/bin/env python3
"""Step time of the single-device fused train step at every active SH degree (gs_set_sh_degree), through
the band-limited forms of the fused projection backward + Adam (GS_TUNE_SH_BAND_SKIP = 1, the default) and through the full-row
form (0), with the stage time of that kernel.

    python tools/sh_degree_step_time.py [--config c3_300k_800] [--views 20] [--steps 200] [--warmup 2] [--profile-steps 40]
                                        [--degrees 0,1,2,3,4] [--timeout 120]

Every (degree, knob) pair runs in a child process of its own under `timeout` (a fresh context and model: the bench scene, K = 25,
densify off so that the count stays put, the degree held by SHDegreeSchedule(start=degree), every view visited --warmup times
before timing); the first child that fails ends the run.  ms per step over --steps steps (device events around the whole loop,
ended by a synchronise), then -- over --profile-steps further steps with the library's stage events on -- the mean gs_profile
time of the fused projection backward + Adam.  At the model's own degree (4) the knob selects nothing: the two runs are the same
kernel, and their difference is the run-to-run spread.  One JSON line: {"config", "N", "steps", "runs": [{"degree", "band_skip",
"ms_per_step", "proj_bwd_adam_ms", "loss"}, ...]}.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(args, degree, knob):
    import torch
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.scenes import CONFIGS, make_config, perturb
    from gaussiansplattingmlx_amd.sh_schedule import SHDegreeSchedule
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    if not torch.cuda.is_available():
        raise SystemExit("sh_degree_step_time: no GPU (a timing taken anywhere else says nothing)")
    idx, N, W, H, _ = CONFIGS[args.config]
    params, cams, _ = make_config(args.config, n_views=args.views)
    r = GaussianRenderer(4, W, H, (16, 16), False)
    r.reserve(N, {0: 2 << 20, 1: 12 << 20, 2: 24 << 20}.get(idx, 96 << 20))
    r.setTuning(sh_band_skip=knob)
    tp = {k: torch.as_tensor(v, device=r.device) for k, v in perturb(params, 12345).items()}
    targets = [r.renderForward(tp, c).render.clone() for c in cams]
    del tp
    V = len(cams)
    model = GaussModel(params, r.device)
    tr = GaussianTrainer(model, r, iterationCount=30000, densify=False, sh_schedule=SHDegreeSchedule(start=degree, every=10 ** 9))
    tr.iteration = 1
    for i in range(args.warmup * V):
        tr.trainStep(cams[i % V], targets[i % V], viewKey=i % V)
    torch.cuda.synchronize()
    assert r.shDegree == degree == tr.lastSHDegree
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(args.steps):
        v = (args.warmup * V + i) % V
        tr.trainStep(cams[v], targets[v], viewKey=v)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / args.steps
    r.profile(("proj_bwd",))
    r.profileRead()
    for i in range(args.profile_steps):
        tr.trainStep(cams[i % V], targets[i % V], viewKey=i % V)
    st = r.profileRead()
    r.profile(False)
    print(json.dumps(dict(degree=degree, band_skip=knob, N=model.N, ms_per_step=round(ms, 4),
                          proj_bwd_adam_ms=round(st["proj_bwd"][0] / max(st["proj_bwd"][1], 1), 4), loss=float(tr._loss[0]))),
          flush=True)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3_300k_800")
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile-steps", type=int, default=40)
    ap.add_argument("--degrees", default="0,1,2,3,4")
    ap.add_argument("--timeout", type=int, default=120, help="seconds per (degree, knob) run")
    ap.add_argument("--one", nargs=2, type=int, metavar=("DEGREE", "KNOB"), help="(a child's run)")
    args = ap.parse_args()
    if args.one:
        return one(args, *args.one)
    runs = []
    for d in (int(x) for x in args.degrees.split(",")):
        for knob in (1, 0):
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--config", args.config,
                   "--views", str(args.views), "--steps", str(args.steps), "--warmup", str(args.warmup), "--profile-steps",
                   str(args.profile_steps), "--one", str(d), str(knob)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:      # (a fault, an abort or the time limit: nothing more is started on the device)
                print(json.dumps(dict(config=args.config, failed=dict(degree=d, band_skip=knob, returncode=p.returncode), runs=runs)),
                      flush=True)
                raise SystemExit(1)
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(runs[-1], file=sys.stderr, flush=True)      # (progress; the result is the one line on stdout)
    N = runs[0].pop("N") if runs else None
    for x in runs[1:]:
        x.pop("N", None)
    print(json.dumps(dict(config=args.config, N=N, steps=args.steps, runs=runs)), flush=True)


if __name__ == "__main__":
    main()
