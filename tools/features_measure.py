#!/usr/bin/env python3
"""What N-channel feature rendering costs on the bench scene.

    python tools/features_measure.py [--channels 3 16 64] [--tag NAME]

One JSON line: gs_render_features and gs_render_features_backward for every channel count, device events around 20 calls
after 3, on the bench scene (c3: 300 k Gaussians, 800 x 800, one view), next to the fused forward (whole call, and its blend
stage) and the fused blend backward (the profiler's blend_bwd stage of renderBackward) of the same view in the same process;
the ratio of the C = 3 feature kernels to the colour blend kernels (the price of the generic payload) and the milliseconds
per channel (whether re-sweeping the list per channel group amortises).  The library under GSPLAT_LIB is measured (an
experiment build of gaussiansplattingmlx_amd.build --variant), --tag names it in the output."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[3, 16, 64])
    ap.add_argument("--tag", default="product")
    args = ap.parse_args()
    import torch
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.scenes import CONFIGS, make_config

    _, N, W, H, _ = CONFIGS["c3_300k_800"]
    params, cams, _ = make_config("c3_300k_800", n_views=1)
    r = GaussianRenderer(4, W, H, (16, 16), False)
    cam = r._camera(cams[0].worldViewTransform, cams[0].projectionMatrix, cams[0].cameraCenter, cams[0].FoVx, cams[0].FoVy,
                    cams[0].focalX, cams[0].focalY)
    p = {k: torch.as_tensor(v, device=r.device) for k, v in params.items()}

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

    fwd = events(lambda: r.renderForward(p, cam, wantDepth=False))
    cot = torch.rand(H, W, 3, device=r.device) - 0.5

    def fwd_bwd():
        r.renderForward(p, cam, wantDepth=False)
        r.renderBackward(cot)
    for _ in range(3):
        fwd_bwd()
    r.profile(("blend_fwd", "blend_bwd"))
    for _ in range(20):
        fwd_bwd()
    st = r.profileRead()
    r.profile(False)
    blend_fwd, blend_bwd = (st[k][0] / max(st[k][1], 1) for k in ("blend_fwd", "blend_bwd"))

    r.renderChecked(p, cam, wantDepth=False)
    M = int(r.stats()["M"])
    gen = torch.Generator(device=r.device).manual_seed(1)
    rows = []
    for C in args.channels:
        f = torch.rand(N, C, device=r.device, generator=gen) * 2 - 1
        ct = torch.rand(H, W, C, device=r.device, generator=gen) * 2 - 1
        out, grad = torch.empty(H, W, C, device=r.device), torch.zeros(N, C, device=r.device)
        f_ms = events(lambda: r.renderFeatures(f, out))
        b_ms = events(lambda: r.renderFeaturesVJP(ct, grad))
        rows.append(dict(C=C, forward_ms=round(f_ms, 4), backward_ms=round(b_ms, 4), forward_ms_per_channel=round(f_ms / C, 5),
                         backward_ms_per_channel=round(b_ms / C, 5)))
    res = dict(measure="render_features", tag=args.tag, group=int(r.lib.gs_feature_channel_group()), scene="c3_300k_800", N=N,
               M=M, fused_forward_ms=round(fwd, 4), fused_blend_forward_ms=round(blend_fwd, 4),
               fused_blend_backward_ms=round(blend_bwd, 4), channels=rows)
    c3 = [x for x in rows if x["C"] == 3]
    if c3:
        res["c3_forward_over_blend_forward"] = round(c3[0]["forward_ms"] / blend_fwd, 3)
        res["c3_backward_over_blend_backward"] = round(c3[0]["backward_ms"] / blend_bwd, 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
