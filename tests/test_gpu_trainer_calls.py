"""The library calls a trainer makes, in order: for every configuration below, the name of every gs_* function that the
constructor, three trainStep calls (the second followed by the configuration's event) or one evaluate / pruneByContribution
call reaches, against tests/golden/trainer_call_sequences.json.  The golden file was recorded with this code on the commit
BEFORE the trainer's shared pieces were gathered, twice, with equal logs:

    python tests/test_gpu_trainer_calls.py OUT.json        # on the commit to pin, on the GPU: writes every configuration's log

Beside the names the log keeps gs_ctx_set_tuning's knob and value and, of the gs_set_* calls, whether each pointer argument is
null.  No address, count or float reaches it.  The blend backward's float atomics are not reproducible run to run (DESIGN.md
section 9), so every host decision that shapes the log is made by a wide margin: a gradient threshold of 0 (everything seen
grows) or 1e30 (nothing does), a block of opacities far below minOpacity (a prune is certain), no pair reserve (no overflow
path), and a scene far too small for a depth cut to miss."""
import ctypes as C
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_call_sequences.json")
W = H = 64
N, DIM = 300, 40          # Gaussians; the first DIM of them all but transparent


class _Recorder:
    """Stands in for renderer.lib: appends what the module's docstring says to `log` and forwards the call."""

    def __init__(self, lib, log, knobs):
        self._lib, self._log, self._knobs = lib, log, {v: k for k, v in knobs.items()}

    @staticmethod
    def _null(a):
        return a is None or (isinstance(a, C.c_void_p) and not a.value) or (isinstance(a, int) and a == 0)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("gs_"):
            return fn

        def call(*a):
            entry = name
            if name == "gs_ctx_set_tuning":
                entry = f"{name}({self._knobs[int(a[1])]}={int(a[2])})"
            elif name.startswith("gs_set_"):
                ptr = [i for i, t in enumerate(fn.argtypes) if i > 0 and (t is C.c_void_p or issubclass(t, C._Pointer))]
                entry = f"{name}({','.join('null' if self._null(a[i]) else 'ptr' for i in ptr)})"
            self._log.append(entry)
            return fn(*a)
        return call


def _scene():
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    rng = np.random.default_rng(7)
    cams = [Camera(W, H, 0.9 * W, 0.92 * W, look_at_c2w(e)) for e in ([2.2, -2.6, 1.7], [2.6, -2.2, 1.5])]
    p = dict(xyz=rng.uniform(-0.6, 0.6, (N, 3)), features_dc=rng.normal(0, 1, (N, 1, 3)),
             features_rest=rng.normal(0, 0.08, (N, 24, 3)), scales=rng.normal(np.log(0.08), 0.3, (N, 3)),
             rotation=rng.normal(0, 1, (N, 4)), opacity=rng.uniform(0.5, 2.0, N))
    p["opacity"][:DIM] = -12.0          # sigmoid = 6e-6: far below minOpacity (0.005), any contribution threshold and MCMC's
    return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}, cams


def _group():
    import torch.distributed as dist
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    return dist.group.WORLD


def _configs():
    """name -> (constructor keywords, what the run does beyond three plain steps)."""
    from gaussiansplattingmlx_amd.adc import ADCConfig
    from gaussiansplattingmlx_amd.background import BackgroundConfig
    from gaussiansplattingmlx_amd.contrib_prune import ContribPruneConfig
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    from gaussiansplattingmlx_amd.sh_schedule import SHDegreeSchedule
    _, cams = _scene()
    event = dict(first=599)              # steps 599, 600, 601: the reference event behind step 600
    dp = dict(group=True, step=dict(stepCameras=[cams[0]]))
    return {
        "fused": (dict(), dict()),
        "unfused": (dict(fuse_adam=False), dict()),
        "no_densify": (dict(densify=False), dict()),
        "reference_planned_grow": (dict(), dict(event, threshold=0.0)),
        "reference_planned_prune": (dict(), dict(event, threshold=1e30)),
        "reference_unplanned_grow": (dict(), dict(event, threshold=0.0, env=dict(GSPLAT_PLANNED_DENSIFY="0"))),
        "reference_unplanned_prune": (dict(), dict(event, threshold=1e30, env=dict(GSPLAT_PLANNED_DENSIFY="0"))),
        # steps 1, 2, 3: the event and the opacity reset behind step 2
        "adc_event_reset": (dict(strategy="adc", adc=ADCConfig(scene_extent=3.0, densify_from=2, densify_interval=2,
                                                                opacity_reset_interval=2)), dict(threshold=0.0)),
        "mcmc_event": (dict(strategy="mcmc", mcmc=MCMCConfig(cap_max=400, refine_start=0, refine_every=2)), dict()),
        "mcmc_unfused": (dict(strategy="mcmc", fuse_adam=False, mcmc=MCMCConfig(cap_max=400, refine_start=0, refine_every=2)), dict()),
        "contrib_prune": (dict(contrib_prune=ContribPruneConfig(threshold=0.001, at=(2,), cameras=list(cams))), dict()),
        "pose_exposure_mask": (dict(pose_opt=True, exposure_opt=True, n_views=4), dict(mask=True)),
        "grid_background_depth": (dict(bilateral_grid=True, bilateral_grid_shape=(4, 4, 2), n_views=4, background=BackgroundConfig(),
                                       depth=DepthConfig(mode="expected")), dict(alpha=True, depth=True)),
        "filter_3d": (dict(filter_3d=True, filter_cameras=list(cams), filter_3d_interval=2), dict()),
        "sparse_adam_fused": (dict(sparse_adam=True), dict()),
        "sparse_adam_unfused": (dict(sparse_adam=True, fuse_adam=False), dict()),
        "sh_schedule": (dict(sh_schedule=SHDegreeSchedule(start=0, every=2)), dict()),
        "two_views": (dict(views_per_rank=2), dict(views=2)),
        "dp_sh_compressed_fused": (dict(dp_exchange="sh_compressed", exchange_when_single=True), dp),
        "dp_sh_compressed_unfused": (dict(dp_exchange="sh_compressed", exchange_when_single=True, fuse_adam=False), dp),
        "dp_allreduce": (dict(dp_exchange="allreduce", exchange_when_single=True), dp),
        "evaluate": (dict(pose_opt=True, exposure_opt=True, n_views=4, filter_3d=True, filter_cameras=list(cams),
                          sh_schedule=SHDegreeSchedule(start=1, every=1000)), dict(call="evaluate")),
        "prune_by_contribution": (dict(densify=False), dict(call="prune")),
    }


CONFIGS = ["fused", "unfused", "no_densify", "reference_planned_grow", "reference_planned_prune", "reference_unplanned_grow",
           "reference_unplanned_prune", "adc_event_reset", "mcmc_event", "mcmc_unfused", "contrib_prune", "pose_exposure_mask",
           "grid_background_depth", "filter_3d", "sparse_adam_fused", "sparse_adam_unfused", "sh_schedule", "two_views",
           "dp_sh_compressed_fused", "dp_sh_compressed_unfused", "dp_allreduce", "evaluate", "prune_by_contribution"]


def _run(name, group=None):
    """The configuration's log."""
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    kw, how = _configs()[name]
    p, cams = _scene()
    r = GaussianRenderer(4, W, H, (16, 16), False)
    lib, log = r.lib, []
    env = how.get("env", {})
    saved = {k: os.environ.get(k) for k in env}
    try:
        dev = {k: torch.as_tensor(v, device=r.device) for k, v in p.items()}
        targets = []
        for c in cams:
            res = r.renderChecked(dev, c)
            targets.append((0.5 * res.render + 0.25).clone())          # (not the model's own image: every gradient is non-zero)
            if c is cams[0]:
                depth, alpha = res.depth.reshape(H, W).clone(), res.alpha.reshape(H, W).clone()
        r.sync()
        os.environ.update(env)
        r.lib = _Recorder(lib, log, r._TUNING)
        if how.get("group"):
            kw = dict(kw, process_group=group)
        tr = GaussianTrainer(GaussModel(p, r.device), r, iterationCount=1000, **kw)
        if "threshold" in how:
            tr.gradientThreshold = how["threshold"]
        if how.get("call") == "evaluate":
            tr.evaluate([cams[0]], [targets[0]], viewKeys=[0])
        elif how.get("call") == "prune":
            st = tr.pruneByContribution(list(cams), threshold=0.001)
            assert st["pruned"] >= DIM and st["kept"] > 0
        else:
            tr.iteration = how.get("first", 1)
            step = dict(how.get("step", {}))
            if how.get("mask"):
                m = torch.full((H, W), 255, dtype=torch.uint8, device=r.device)
                m[:8] = 0
                step["lossMask"] = m
            if how.get("alpha"):
                step["targetAlpha"] = alpha
            if how.get("depth"):
                step["targetDepth"] = depth + 0.5
            n0 = tr.model.N
            for _ in range(3):
                if how.get("views"):
                    tr.trainStep(list(cams), list(targets), viewKey=[0, 1], **step)
                else:
                    tr.trainStep(cams[0], targets[0], viewKey=0, **step)
            r.sync()
            if "threshold" in how or name in ("mcmc_event", "contrib_prune"):
                assert tr.model.N != n0, "the configuration's event did not change the model"
            assert tr.forwardMisses == 0 and tr.overflowRecoveries == 0
        if how.get("group"):
            tr.closeExchange()
    finally:
        r.lib = lib
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        r.close()
    return log


@pytest.fixture(scope="module")
def one_rank_group():
    import torch.distributed as dist
    g = _group()
    yield g
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", CONFIGS)
def test_trainer_makes_the_library_calls_it_made(name, golden, request):
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box")
    assert sorted(golden) == sorted(CONFIGS)
    group = request.getfixturevalue("one_rank_group") if _configs()[name][1].get("group") else None
    got, want = _run(name, group), golden[name]
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, f"{name}: {len(got)} calls against {len(want)}; the first difference is at call {first}: " \
                        f"{got[max(first - 3, 0):first + 3]} against {want[max(first - 3, 0):first + 3]}"
    assert not any("0x" in e for e in got)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    grp = _group()
    logs = {}
    for cfg in CONFIGS:
        logs[cfg] = _run(cfg, grp)
        print(cfg, len(logs[cfg]), "calls", flush=True)
    dist.destroy_process_group()
    with open(sys.argv[1], "w") as f:
        json.dump(logs, f, indent=0)
        f.write("\n")
