"""The active SH degree on the device (include/gsplat.h gs_set_sh_degree): forwards and the unfused
backward at a lower degree against the float32 oracle at that degree, one fused step through the band-limited forms of
proj_bwd_fused_kernel (csrc/projection.hip, BANDS) against the same step through the full-row form (sh_band_skip = 0), the forms
that do not skip, ten scheduled trainer steps against an oracle-driven loop, the overflow gate, the ranges, and that off is off.

Scenes and cameras are those of tests/test_sparse_adam_cpu.py (scene(N, K): camera A sees every Gaussian, camera B stands inside
the cloud); K = 9 is the same scene cut to 8 rest rows.  Lact = 3 ((d + 1)^2 - 1) columns of a features_rest row (flattened
[K - 1, 3], L = 3 (K - 1)) are active at degree d: 0, 9, 24, 45.  At L = 72 the 16-byte word over columns 8..11 straddles Lact at
d = 1 and the one over 44..47 at d = 3, d = 2 cuts between two words; L = 45 and L = 9 go element by element; 3000 = 46 waves + a
tail of 56 rows, 3001 one of 57.

Bars.  Inactive columns: bit-identical in the parameter and both moment arenas.  Everything else, two device runs against each
other (the blend backward's float atomics are not bit-reproducible from run to run): the share bar of
test_fused_backward_adam_matches_backward_then_adam, mean(|a - b| > 1e-3 max|b|) < 1e-3 per tensor, the parameters compared as
their change over the step.  Forward: 1e-4 L-inf against the float32 oracle; unfused gradients: test_gpu_parity's 1e-3 of the
tensor's largest magnitude.  Trajectory: the bars of tests/test_gpu_trajectory.py, computed as there.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from gaussiansplattingmlx_amd import sparse_adam as sa
from gaussiansplattingmlx_amd.sh_schedule import SHDegreeSchedule, active_columns

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")
W, H = 160, 120
SHARE_TOL, SHARE = 1e-3, 1e-3
RGB_TOL, GRAD_RTOL = 1e-4, 1e-3
DEGREE = {25: 4, 16: 3, 9: 2, 4: 1}


def _load(name):
    spec = importlib.util.spec_from_file_location("_shd_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cpu = _load("test_sparse_adam_cpu")
traj = _load("test_gpu_trajectory")


def _renderer(K=25, aa=False):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(DEGREE[K], W, H, (16, 16), False, antialiased=aa)


def _dev(p):
    return {k: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32, device="cuda") for k, v in p.items()}


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cot():
    """The colour cotangent of test_absgrad_cpu.cotangents("plain")."""
    return torch.as_tensor((np.random.default_rng(3).standard_normal((H, W, 3)) / (W * H)).astype(np.float32), device="cuda")


def _rows(model, name):
    return {k: _np(v).copy() for k, v in model._carve(getattr(model, name), model.N, model.stride).items()}


def _state(model):
    return {name: _rows(model, name) for name in ("arena", "m", "v")}


def _rest(model, name):
    """features_rest of one of the model's buffers as a writable [N, L] device view."""
    v = model._carve(getattr(model, name), model.N, model.stride)["features_rest"]
    return v.view(model.N, -1)


def _share(a, b):
    return float(np.mean(np.abs(a - b) > SHARE_TOL * np.abs(b).max())) if b.size else 0.0


def _assert_inactive_bits(after, before, lact, what):
    for name in ("arena", "m", "v"):
        a = after[name]["features_rest"].reshape(after[name]["features_rest"].shape[0], -1)[:, lact:]
        b = before[name]["features_rest"].reshape(a.shape[0], -1)[:, lact:]
        assert np.array_equal(_bits(a), _bits(b)), (what, name, int((_bits(a) != _bits(b)).sum()))


def _assert_rest_close(got, want, start, lact, what):
    """Per tensor, the share bar over everything but the inactive columns: the parameters as their change over the step."""
    for name in ("arena", "m", "v"):
        for k in KEYS:
            a, b = got[name][k].astype(np.float64), want[name][k].astype(np.float64)
            s = start["arena"][k].astype(np.float64)
            if k == "features_rest":
                a, b, s = (x.reshape(x.shape[0], -1)[:, :lact] for x in (a, b, s))
            if name == "arena":
                a, b = a - s, b - s
            sh = _share(a, b)
            print(f"{what} {name}.{k}: share of elements further than {SHARE_TOL:.0e} max|b| = {sh:.2e} (bar {SHARE:.0e})")
            assert sh < SHARE, (what, name, k)
            if a.size:
                assert np.abs(b).max() > 0, (what, name, k)          # the step moved the tensor


def _restore(model, clone):
    for name in ("arena", "m", "v"):
        getattr(model, name).copy_(clone[name])


def _targets(r, p, cams):
    from gaussiansplattingmlx_amd.scenes import perturb
    tp = _dev(perturb(p, 5, 0.1))
    return [r.renderChecked(tp, c).render.clone() for c in cams]


# ---------------------------------------------------------------------------------------------------------------- 1. forward
def test_forward_matches_the_oracle_at_every_degree(oracle32):
    N, K = 3000, 25
    p, cams = cpu.scene(N, K)
    params = _dev(p)
    r0 = _renderer(K)                                       # never hears of the setter
    full = r0.renderForward(params, cams[0]).render.clone()
    r = _renderer(K)
    assert r.shDegree == r.maxSHDegree == r.active_sh_degree == 4
    imgs = []
    for d in (0, 1, 2, 3):
        r.setSHDegree(d)
        assert r.shDegree == d and r.active_sh_degree == 4
        img = _np(r.renderForward(params, cams[0]).render).reshape(-1, 3)
        want = oracle32.render_forward(p, cams[0].as_dict(), W, H, 16, 16, d)["color"]
        err = float(np.abs(img - want).max())
        print(f"degree {d}: RGB L-inf against the float32 oracle {err:.2e} (bar {RGB_TOL:.0e})")
        assert err <= RGB_TOL
        imgs.append(img.copy())
    for a, b in zip(imgs, imgs[1:]):
        assert np.abs(a - b).max() > 1e-3                   # the bands are visible in this scene
    r.shDegree = 4
    assert torch.equal(r.renderForward(params, cams[0]).render, full)


# ------------------------------------------------------------------------------------------------------- 2. unfused backward
@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_unfused_backward_matches_the_oracle(oracle32, d):
    N, K = 3000, 25
    p, cams = cpu.scene(N, K)
    lact = active_columns(d)
    r = _renderer(K)
    r.setSHDegree(d)
    r.renderForward(_dev(p), cams[0])
    cot = _cot()
    got = r.renderBackward(cot)
    rest = _np(got["features_rest"]).reshape(N, -1)
    assert not _bits(rest[:, lact:]).any()                  # exactly 0.0
    c = cams[0].as_dict()
    fw = oracle32.render_forward(p, c, W, H, 16, 16, d)
    z = np.zeros(W * H, np.float32)
    want = oracle32.render_backward(p, c, W, H, 16, 16, d, fw, _np(cot).reshape(-1, 3), z, z)
    for k in KEYS:
        a, b = _np(got[k]).astype(np.float64), np.asarray(want[k], np.float64).reshape(_np(got[k]).shape)
        rel = float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))
        print(f"degree {d} {k}: {rel:.2e} of the largest magnitude {np.abs(b).max():.2e} (bar {GRAD_RTOL:.0e})")
        assert rel <= GRAD_RTOL, k
        assert np.abs(b).max() > 0 or (k == "features_rest" and d == 0)


# --------------------------------------------------------------------------------------------------- 3. one fused BANDS step
CASES = [(3000, 25, 0, {}), (3000, 25, 1, {}), (3000, 25, 2, {}), (3000, 25, 3, {}), (3001, 25, 1, {}), (1500, 16, 0, {}),
         (1500, 16, 1, {}), (1500, 16, 2, {}), (900, 9, 1, {}), (700, 4, 0, {}), (3000, 25, 1, dict(aa=True)),
         (3000, 25, 3, dict(fisheye=True))]


def _case_id(c):
    return f"{c[0]}-{c[1]}-d{c[2]}" + "".join("-" + k for k in c[3])


def _pattern(n, cols, seed):
    """A distinctive non-zero pattern: no element is 0, none repeats along a row."""
    rng = np.random.default_rng(seed)
    return torch.as_tensor((0.25 + rng.random((n, cols))).astype(np.float32) * (1 + np.arange(cols, dtype=np.float32))[None, :],
                           device="cuda")


@pytest.mark.parametrize("N,K,d,opt", CASES, ids=[_case_id(c) for c in CASES])
def test_one_fused_bands_step(N, K, d, opt):
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    from gaussiansplattingmlx_amd.trainer import GaussModel, getLearningRates
    p, cams = cpu.scene(N, K)
    L, lact = 3 * (K - 1), active_columns(d)
    assert lact < L and (d + 2) ** 2 <= K
    camA, camB = cams[0], cams[1]
    if opt.get("fisheye"):
        camA, camB = (Camera(W, H, 144, 144 * 1.02, look_at_c2w(e), model="fisheye") for e in ([2.2, -2.6, 1.7], [0.4, -0.5, 0.3]))
    r = _renderer(K, aa=bool(opt.get("aa")))
    model = GaussModel(p, r.device)
    lrs = getLearningRates(0, 1000)
    cot = _cot()
    # moments everywhere: one full-degree step on camera A, which sees every Gaussian
    r.renderForward(model.getParams(), camA, wantDepth=False)
    r.renderBackwardAdam(cot, model.arena, model.m, model.v, lrs)
    assert bool((_rest(model, "m")[:, lact:] != 0).any())
    r.setSHDegree(d)
    base = {name: getattr(model, name).clone() for name in ("arena", "m", "v")}
    banded = {}
    for variant in ("pattern", "nan"):
        _restore(model, base)
        _rest(model, "arena")[:, lact:] = _pattern(N, L - lact, 1)
        if variant == "pattern":
            _rest(model, "m")[:, lact:] = -_pattern(N, L - lact, 2)
            _rest(model, "v")[:, lact:] = _pattern(N, L - lact, 3)
        else:
            _rest(model, "m")[:, lact:] = float("nan")
            _rest(model, "v")[:, lact:] = float("nan")
        start = _state(model)
        clone = {name: getattr(model, name).clone() for name in ("arena", "m", "v")}
        r.renderForward(model.getParams(), camB, wantDepth=False)
        r.renderBackwardAdam(cot, model.arena, model.m, model.v, lrs)
        banded[variant] = _state(model)
        # (a) the inactive columns: every bit, in all three arenas -- and the pads and everything else outside the six tensors
        _assert_inactive_bits(banded[variant], start, lact, f"{variant} banded")
        if lact:
            act = banded[variant]["arena"]["features_rest"].reshape(N, -1)[:, :lact]
            assert (_bits(act) != _bits(start["arena"]["features_rest"].reshape(N, -1)[:, :lact])).mean() > 0.5
        assert np.isfinite(banded[variant]["arena"]["features_rest"]).all()
        # the pads between the tensors were never written
        on = sa.element_mask(np.ones(N, bool), model.seg_end, sa.model_row_floats(model), N)
        for name in ("arena", "m", "v"):
            assert np.array_equal(_bits(_np(getattr(model, name))[~on]), _bits(_np(clone[name])[~on])), name
    # (b) the same step through the full-row form, the inactive moments zeroed for it
    _restore(model, clone)
    _rest(model, "m")[:, lact:] = 0.0
    _rest(model, "v")[:, lact:] = 0.0
    start0 = _state(model)
    r.setTuning(sh_band_skip=0)
    r.renderForward(model.getParams(), camB, wantDepth=False)
    r.renderBackwardAdam(cot, model.arena, model.m, model.v, lrs)
    r.setTuning(sh_band_skip=1)
    full = _state(model)
    _assert_inactive_bits(full, start0, lact, "full-row form on zero moments")        # the invariant of DESIGN section 30
    for variant in ("pattern", "nan"):
        _assert_rest_close(banded[variant], full, start, lact, f"{_case_id((N, K, d, opt))} {variant}")


def test_an_overflowed_bands_step_moves_nothing():
    """Arranged as test_gpu_sparse_adam.test_an_overflowed_step_moves_no_row."""
    from gaussiansplattingmlx_amd._lib import GsplatError
    from gaussiansplattingmlx_amd.trainer import GaussModel
    N, K, d = 3000, 25, 1
    p, cams = cpu.scene(N, K)
    r0 = _renderer(K)
    r0.renderForward(_dev(p), cams[1])
    r0.sync()
    M = r0.stats()["M"]
    r0.close()
    r = _renderer(K)
    r.reserve(N, M // 3)                                     # too small on purpose: a reported overflow
    r.setSHDegree(d)
    model = GaussModel(p, r.device)
    model.m.fill_(0.25)
    model.v.fill_(0.125)
    before = {name: getattr(model, name).clone() for name in ("arena", "m", "v")}
    res = r.renderForward(model.getParams(), cams[1], wantDepth=False)
    try:                                                     # may or may not have seen the flag yet: both are in contract
        _, gc, _ = r.lossForwardBackward(res.render, torch.rand(H, W, 3, device="cuda"), 0.2)
        r.renderBackwardAdam(gc, model.arena, model.m, model.v, [1e-2] * 6)
    except GsplatError as e:
        assert e.code == 3
    with pytest.raises(GsplatError) as ei:
        r.sync()
    assert ei.value.code == 3 and r.stats()["overflow"] == 1
    for name in ("arena", "m", "v"):
        assert torch.equal(getattr(model, name), before[name]), name


# --------------------------------------------------------------------------------------------- 4. the forms that do not skip
@pytest.mark.parametrize("feature", ["sparse_adam", "mcmc", "pose_opt"])
def test_full_row_forms_leave_zero_moment_bands_alone(feature):
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    N, K, d = 1500, 16, 1
    p, cams = cpu.scene(N, K)
    lact = active_columns(d)
    r = _renderer(K)
    targets = _targets(r, p, cams)
    model = GaussModel(p, r.device)
    kw = dict(sparse_adam=dict(sparse_adam=True, densify=False), mcmc=dict(strategy="mcmc", mcmc=MCMCConfig(cap_max=N)),
              pose_opt=dict(pose_opt=True, n_views=3, densify=False))[feature]
    tr = GaussianTrainer(model, r, iterationCount=1000, sh_schedule=SHDegreeSchedule(start=d, every=1000), **kw)
    start = _state(model)
    loss = tr.trainStep(cams[0], targets[0], viewKey=0)
    assert np.isfinite(_np(loss)).all() and tr.lastSHDegree == d and r.shDegree == d
    after = _state(model)
    assert after["arena"]["features_rest"].shape == start["arena"]["features_rest"].shape      # (no event in the first step)
    _assert_inactive_bits(after, start, lact, feature)
    assert not _bits(after["m"]["features_rest"].reshape(N, -1)[:, lact:]).any()
    act = lambda s: s["arena"]["features_rest"].reshape(N, -1)[:, :lact]      # noqa: E731
    assert (_bits(act(after)) != _bits(act(start))).mean() > 0.5             # the active bands trained


# ---------------------------------------------------------------------------------------------------------------- 5. trajectory
def _oracle_loop(o, p0, cams, targets, schedule, steps, lam=0.2):
    """tests/test_gpu_trajectory.py's _oracle_loop with the schedule's degree handed to the oracle."""
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, getLearningRates
    dt = o.dtype
    p = {k: v.astype(dt).copy() for k, v in p0.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    b1, b2, eps, one = dt.type(0.9), dt.type(0.999), dt.type(1e-15), dt.type(1)
    z = np.zeros(W * H, dt)
    losses = []
    for it in range(steps):
        d = schedule.degree_at(it, 4)
        cam = cams[it % len(cams)].as_dict()
        fw = o.render_forward(p, cam, W, H, 16, 16, d)
        loss, cot, _, _, _ = o.loss_forward_backward(fw["color"].reshape(H, W, 3), targets[it % len(cams)].astype(dt), lam)
        g = o.render_backward(p, cam, W, H, 16, 16, d, fw, cot.reshape(-1, 3), z, z)
        losses.append(loss)
        lr = dict(zip(PARAM_ORDER, getLearningRates(it, traj.TOTAL)))
        for k in KEYS:
            gk = np.asarray(g[k], dt).reshape(p[k].shape)
            m[k] = b1 * m[k] + (one - b1) * gk
            v[k] = b2 * v[k] + (one - b2) * gk * gk
            p[k] = (p[k] - dt.type(lr[k]) * m[k] / (np.sqrt(v[k]) + eps)).astype(dt)
    return losses, p, m, v


def test_scheduled_trajectory_matches_the_oracle_loop(oracle32, oracle64):
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, GaussianTrainer, GaussModel, getLearningRates
    N, STEPS = 3000, traj.STEPS
    sched = SHDegreeSchedule(every=3)
    table = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]
    assert [sched.degree_at(t, 4) for t in range(STEPS)] == table
    p0, cams = traj._scene(71, N, W, H, 0.06)
    tp = perturb(p0, 5, 0.1)
    targets = [oracle32.render_forward(tp, c.as_dict(), W, H, 16, 16, 4)["color"].reshape(H, W, 3).copy() for c in cams]
    want_l, want_p, want_m, want_v = _oracle_loop(oracle32, p0, cams, targets, sched, STEPS)
    ref_l, ref_p, _, _ = _oracle_loop(oracle64, p0, cams, targets, sched, STEPS)
    r = _renderer(25)
    model = GaussModel(p0, r.device)
    tr = GaussianTrainer(model, r, iterationCount=traj.TOTAL, densify=False, sh_schedule=sched)
    tg = [torch.as_tensor(t, device=r.device) for t in targets]
    first = _state(model)
    got_l = []
    for it in range(STEPS):
        v = it % len(cams)
        got_l.append(float(tr.trainStep(cams[v], tg[v], viewKey=v, stepCameras=[cams[v]])[0]))
        assert tr.lastSHDegree == table[it] == r.shDegree
        _assert_inactive_bits(_state(model), first, active_columns(table[it]), f"step {it}")
    assert r.stats()["overflow"] == 0 and tr.forwardMisses == 0
    got_p = {k: _np(model.getParams()[k]).copy() for k in KEYS}
    got_m = {k: _np(model._carve(model.m, N)[k]).copy() for k in KEYS}
    got_v = {k: _np(model._carve(model.v, N)[k]).copy() for k in KEYS}
    report = {}
    traj._compare("param", got_p, want_p, p0, report)
    traj._compare("m", got_m, want_m, p0, report)
    traj._compare("v", got_v, want_v, p0, report)
    traj._compare("oracle32_vs_64.param", {k: ref_p[k] for k in KEYS}, want_p, p0, report)
    dl = np.abs(np.asarray(got_l) - np.asarray(want_l))
    print("loss |hip - oracle32| per step:", [f"{x:.1e}" for x in dl], "oracle64:", [f"{abs(a - b):.1e}" for a, b in zip(ref_l, want_l)])
    for k, e in report.items():
        print(k, e)
    assert got_l[-1] < got_l[0]
    assert dl.max() <= traj.LOSS_TOL, (dl.tolist(), got_l, want_l)
    lr = dict(zip(PARAM_ORDER, getLearningRates(0, traj.TOTAL)))
    for k in KEYS:
        for tag in ("m", "v"):
            e = report[f"{tag}.{k}"]
            assert e["share_beyond"] <= traj.MOMENT_SHARE and e["max_rel"] <= 2e-2, (tag, k, e)
        e, ref = report[f"param.{k}"], report[f"oracle32_vs_64.param.{k}"]
        assert e["share_beyond"] <= 1.5 * ref["share_beyond"] + 5e-4, (k, e, ref)
        assert e["max_abs"] <= 2 * 3.17 * lr[k] * STEPS * 1.01 + 1e-6, (k, e)
    # the oracle loop leaves the bands that never became active where they started, too
    assert np.array_equal(_bits(want_p["features_rest"].reshape(N, -1)[:, 45:]), _bits(p0["features_rest"].reshape(N, -1)[:, 45:]))


# ---------------------------------------------------------------------------------------------------------------- 6. off is off
def test_off_is_off():
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    N, K = 3000, 25
    p, cams = cpu.scene(N, K)
    runs = []
    for kw in ({}, dict(sh_schedule=None)):
        r = _renderer(K)
        targets = _targets(r, p, cams)
        model = GaussModel(p, r.device)
        tr = GaussianTrainer(model, r, iterationCount=1000, densify=False, **kw)
        assert tr.sh_schedule is None
        calls = []
        for it in range(4):
            r.profile(True)
            tr.trainStep(cams[it % 3], targets[it % 3], viewKey=it % 3)
            calls.append({k: n for k, (_, n) in r.profileRead().items()})
        r.profile(False)
        assert tr.lastSHDegree is None and r.shDegree == r.maxSHDegree == 4 and r.getTuning("sh_band_skip") == 1
        d = C.c_int(-1)
        assert r.lib.gs_get_sh_degree(r.ctx, C.byref(d)) == 0 and d.value == 4
        runs.append((calls, _state(model)))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])          # stage for stage, call for call
    assert all(c["proj_bwd"] == 1 and c["blend_bwd"] == 1 for c in runs[0][0]), runs[0][0]
    # the full-degree step moves every band: no column of features_rest is left alone
    moved = (_bits(runs[0][1]["arena"]["features_rest"]) != _bits(p["features_rest"])).reshape(N, -1).any(axis=0)
    assert moved.all()


# ------------------------------------------------------------------------------------------------- 7. refusals and ranges
def test_setter_ranges_and_the_k_check():
    import ctypes as C
    from gaussiansplattingmlx_amd._lib import GsplatError
    p25, cams = cpu.scene(3000, 25)
    p16, _ = cpu.scene(1500, 16)
    r = _renderer(25)
    for bad in (-1, 5, 100):
        assert r.lib.gs_set_sh_degree(r.ctx, bad) == 1
        assert r.lib.gs_last_error(r.ctx).decode().startswith("gs_set_sh_degree:")
        assert r.shDegree == 4
    assert r.lib.gs_get_sh_degree(r.ctx, None) == 1
    with pytest.raises(GsplatError):
        r.setSHDegree(5)
    with pytest.raises(ValueError):
        r.setSHDegree(1.5)
    r3 = _renderer(16)
    assert r3.lib.gs_set_sh_degree(r3.ctx, 4) == 1 and r3.shDegree == r3.maxSHDegree == 3
    # every K check uses the active degree: a K = 16 model on a degree-4 context is refused at 4 and served at 3
    with pytest.raises(GsplatError) as ei:
        r.renderForward(_dev(p16), cams[0])
    assert ei.value.code == 2
    r.setSHDegree(3)
    img = r.renderForward(_dev(p16), cams[0]).render
    assert torch.equal(img, r3.renderForward(_dev(p16), cams[0]).render)
    d = C.c_int(-1)
    assert r.lib.gs_get_sh_degree(r.ctx, C.byref(d)) == 0 and d.value == 3


def test_a_backward_uses_the_degree_of_its_forward():
    N, K = 3000, 25
    p, cams = cpu.scene(N, K)
    r = _renderer(K)
    params, cot = _dev(p), _cot()
    r.setSHDegree(1)
    r.renderForward(params, cams[0])
    want = _np(r.renderBackward(cot)["features_rest"]).reshape(N, -1).copy()
    r.renderForward(params, cams[0])
    r.setSHDegree(3)
    got = _np(r.renderBackward(cot)["features_rest"]).reshape(N, -1)
    assert not _bits(got[:, 9:]).any() and not _bits(want[:, 9:]).any()
    assert (np.abs(got[:, :9]).max(axis=0) > 0).all()
    assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()      # (float atomics: test_forward_without_a_depth_image's bar)
    # ... and the fused Adam step too: a degree-1 forward, the degree raised, the step leaves the columns from 9 on alone
    from gaussiansplattingmlx_amd.trainer import GaussModel, getLearningRates
    model = GaussModel(p, r.device)
    _rest(model, "m")[:, 9:] = 0.5
    start = _state(model)
    r.setSHDegree(1)
    r.renderForward(model.getParams(), cams[0], wantDepth=False)
    r.setSHDegree(3)
    r.renderBackwardAdam(cot, model.arena, model.m, model.v, getLearningRates(0, 1000))
    _assert_inactive_bits(_state(model), start, 9, "forward at 1, step at 3")
