"""Which argument sets GaussianTrainer's constructor refuses, and with which message: the default arguments, every single
feature switch and every pair of switches, against tests/golden/trainer_refusals.json.  The golden file was recorded with
this enumeration on the commit BEFORE the constructor's validation was gathered into one table, so it
pins the first message raised for every argument set to what it was:

    python tests/test_trainer_refusals_cpu.py        # on the commit to pin: rewrites the golden file

The model is a stub with only N, and there is no renderer: an argument set that passes validation fails at the first touch
of either (any exception but a ValueError), which counts as "passed validation"."""
import itertools
import json
import os
import sys
import types

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_refusals.json")
PASSED = "passed validation"


def _switches():
    from gaussiansplattingmlx_amd.absgrad import AbsGradConfig
    from gaussiansplattingmlx_amd.adc import ADCConfig
    from gaussiansplattingmlx_amd.background import BackgroundConfig
    from gaussiansplattingmlx_amd.contrib_prune import ContribPruneConfig
    from gaussiansplattingmlx_amd.depth_loss import DepthConfig
    from gaussiansplattingmlx_amd.sh_schedule import SHDegreeSchedule
    cam = object()      # (validation only counts the cameras)
    return {
        "pose_opt": dict(pose_opt=True, n_views=4),
        "exposure_opt": dict(exposure_opt=True, n_views=4),
        "bilateral_grid": dict(bilateral_grid=True, n_views=4),
        "filter_3d": dict(filter_3d=True, filter_cameras=[cam]),
        "sparse_adam": dict(sparse_adam=True),
        "adc": dict(strategy="adc", adc=ADCConfig(scene_extent=1.0)),
        "mcmc": dict(strategy="mcmc"),
        "absgrad": dict(absgrad=AbsGradConfig()),
        "background": dict(background=BackgroundConfig()),
        "depth": dict(depth=DepthConfig()),
        "sh_schedule": dict(sh_schedule=SHDegreeSchedule()),
        "contrib_prune": dict(contrib_prune=ContribPruneConfig(cameras=[cam])),
        "views_per_rank": dict(views_per_rank=2),
        "native": dict(exchange_impl="native", dp_bootstrap=(b"", 0, 1)),
        "no_densify": dict(densify=False),
        "allreduce": dict(dp_exchange="allreduce"),
    }


def _outcome(kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    try:
        GaussianTrainer(types.SimpleNamespace(N=1), None, **kw)
    except ValueError as e:
        return str(e)
    except Exception:
        return PASSED
    return PASSED


def enumerate_outcomes():
    sw = _switches()
    out = {"": _outcome({})}
    for name, kw in sw.items():
        out[name] = _outcome(kw)
    for a, b in itertools.combinations(sw, 2):
        ka, kb = sw[a], sw[b]
        if any(k in kb and kb[k] != ka[k] for k in ka):
            continue        # (two values for one keyword -- strategy="adc" and strategy="mcmc" -- are no argument set)
        out[f"{a}+{b}"] = _outcome({**ka, **kb})
    return out


def test_constructor_refuses_what_it_refused_and_says_what_it_said():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = enumerate_outcomes()
    assert len(want) == 136 and sum(v != PASSED for v in want.values()) == 36
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = enumerate_outcomes()
    with open(GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(res), "cases,", sum(v != PASSED for v in res.values()), "refusals")
