"""The MCMC strategy on the device (include/gsplat.h gs_set_mcmc, gs_mcmc_*) against the numpy
restatement in tests/mcmc_numpy.py and the float64 formula of gaussiansplattingmlx_amd.mcmc.

Bars, fixed before the first run: the regulariser op 1e-6 relative (float32 sigmoid and exp of a float64 statement); the
generator's words exactly, its uniforms exactly (the same IEEE operations), its normals 1e-5 absolute (float32 logf / sincosf);
the noise op 1e-5 of the largest component; one fused step against the unfused one and against a numpy step from the oracle's
gradients, test_gpu_trajectory's bars; the event's opacity and scale 1e-6 relative to the float64 formula, every other row bit
for bit; the default non-interference bit for bit; the trajectory test_gpu_trajectory's bars on the rows the event did not touch.
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")


def _load(name):
    spec = importlib.util.spec_from_file_location("_mcmcg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mn = _load("mcmc_numpy")
traj = _load("test_gpu_trajectory")


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box")


def _renderer(W=160, H=120, aa=False):
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(4, W, H, (16, 16), False, antialiased=aa)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _rows(seed, N, K=16):
    rng = np.random.default_rng(seed)
    p = dict(xyz=rng.uniform(-1, 1, (N, 3)), features_dc=rng.normal(0, 1, (N, 1, 3)),
             features_rest=rng.normal(0, 0.01, (N, K - 1, 3)), scales=rng.normal(-3, 0.7, (N, 3)),
             rotation=rng.normal(0, 1, (N, 4)), opacity=rng.normal(-1, 2.5, N))
    return {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}


# ---------------------------------------------------------------------------------------------------------- per-step ops
def test_regularizer_op_matches_float64():
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    _gpu()
    r = _renderer()
    p = _rows(1, 5000)
    gs = torch.as_tensor(np.random.default_rng(2).normal(0, 1e-4, (5000, 3)).astype(np.float32), device="cuda")
    go = torch.as_tensor(np.random.default_rng(3).normal(0, 1e-4, 5000).astype(np.float32), device="cuda")
    gs0, go0 = _np(gs).astype(np.float64), _np(go).astype(np.float64)
    cfg = MCMCConfig(opacity_reg=0.01, scale_reg=0.02)
    r.mcmcRegularizerGrad(torch.as_tensor(p["scales"], device="cuda"), torch.as_tensor(p["opacity"], device="cuda"), gs, go,
                          cfg.params(0, 1))
    ws, wo = mn.regularizer_grads(p["scales"], p["opacity"], 0.01, 0.02)
    for got, base, add in ((_np(gs), gs0, ws), (_np(go), go0, wo)):       # added: within the float32 rounding of the sum
        assert (np.abs(got - (base + add)) <= 1.2e-7 * np.abs(base + add) + 1e-6 * np.abs(add)).all()
    zs, zo = torch.zeros_like(gs), torch.zeros_like(go)                   # alone: 1e-6 relative
    r.mcmcRegularizerGrad(torch.as_tensor(p["scales"], device="cuda"), torch.as_tensor(p["opacity"], device="cuda"), zs, zo,
                          cfg.params(0, 1))
    for got, want in ((_np(zs), ws), (_np(zo), wo)):
        assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), (np.abs(got - want) / np.abs(want)).max()


@pytest.mark.parametrize("stream", [0, 1, 2])
def test_generator_matches_the_restatement(stream):
    _gpu()
    r = _renderer()
    n, seed, t = 4096, 0x1234_5678_9ABC_DEF0, 700 + stream
    words, normals, uniforms = r.mcmcRandom(seed, t, stream, n)
    want = mn.philox(np.arange(n), t, stream, seed)
    np.testing.assert_array_equal(_np(words).view(np.uint32), want)
    np.testing.assert_array_equal(_np(uniforms), mn.uniforms(want))
    assert np.abs(_np(normals).astype(np.float64) - mn.normals(want)).max() <= 1e-5
    z = mn.normals(want)
    assert abs(z.mean()) < 0.05 and abs(z.std() - 1) < 0.05


def test_noise_op_matches_numpy():
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    _gpu()
    r = _renderer()
    N = 6000
    p = _rows(4, N)
    p["opacity"][:2000] = np.random.default_rng(5).uniform(-7, -4, 2000).astype(np.float32)    # o ~ 0.001 .. 0.02: the gate open
    d = {k: torch.as_tensor(v, device="cuda") for k, v in p.items()}
    cfg = MCMCConfig()
    lr, t, seed = 1.6e-4, 812, 99
    r.mcmcInjectNoise(d["xyz"], d["scales"], d["rotation"], d["opacity"], lr, cfg.params(t, seed))
    eps = mn.normals(mn.philox(np.arange(N), t, 0, seed))
    want = mn.noise(p["scales"], p["rotation"], p["opacity"], eps, cfg.noise_lr, np.float32(lr).astype(np.float64))
    got = _np(d["xyz"]).astype(np.float64) - p["xyz"]
    assert np.abs(want).max() > 1e-3                            # (the gate is open somewhere)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), np.abs(got - want).max()
    # gated (the context's update gate raised): nothing moves
    gate = torch.ones(1, dtype=torch.int32, device="cuda")
    r._check(r.lib.gs_set_update_gate(r.ctx, gate.data_ptr()))
    before = d["xyz"].clone()
    r.mcmcInjectNoise(d["xyz"], d["scales"], d["rotation"], d["opacity"], lr, cfg.params(t + 1, seed))
    r._check(r.lib.gs_set_update_gate(r.ctx, None))
    assert torch.equal(before, d["xyz"])


# ---------------------------------------------------------------------------------------------------------- one step
def _mcmc_trainer(r, p0, cfg, **kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    model = GaussModel(p0, r.device)
    return GaussianTrainer(model, r, iterationCount=traj.TOTAL, strategy="mcmc", mcmc=cfg, **kw), model


def _state(model):
    N = model.N
    return ({k: _np(model.getParams()[k]) for k in KEYS}, {k: _np(model._carve(model.m, N, model.stride)[k]) for k in KEYS},
            {k: _np(model._carve(model.v, N, model.stride)[k]) for k in KEYS})


def _numpy_step(o, p, m, v, cam, target, W, H, it, cfg, seed, lam=0.2):
    """One step of the strategy on the CPU: the oracle's gradients + the regularisers, float32 Adam, the noise in float64."""
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, getLearningRates
    dt = np.float32
    z = np.zeros(W * H, dt)
    fw = o.render_forward(p, cam.as_dict(), W, H, 16, 16, 4)
    loss, cot, _, _, _ = o.loss_forward_backward(fw["color"].reshape(H, W, 3), target.astype(dt), lam)
    g = o.render_backward(p, cam.as_dict(), W, H, 16, 16, 4, fw, cot.reshape(-1, 3), z, z)
    g = {k: np.asarray(g[k], np.float64).reshape(p[k].shape) for k in KEYS}
    rs, ro = mn.regularizer_grads(p["scales"], p["opacity"], cfg.opacity_reg, cfg.scale_reg)
    g["scales"] += rs
    g["opacity"] += ro
    lr = dict(zip(PARAM_ORDER, getLearningRates(it, traj.TOTAL)))
    b1, b2, eps, one = dt(0.9), dt(0.999), dt(1e-15), dt(1)
    for k in KEYS:
        gk = g[k].astype(dt)
        m[k] = b1 * m[k] + (one - b1) * gk
        v[k] = b2 * v[k] + (one - b2) * gk * gk
        p[k] = (p[k] - dt(lr[k]) * m[k] / (np.sqrt(v[k]) + eps)).astype(dt)
    e = mn.normals(mn.philox(np.arange(p["xyz"].shape[0]), it, 0, seed))
    p["xyz"] = (p["xyz"] + mn.noise(p["scales"], p["rotation"], p["opacity"], e, cfg.noise_lr,
                                    float(np.float32(lr["xyz"])))).astype(dt)
    return float(loss)


def _scene_with_dim_rows(N=3000, W=160, H=120):
    p0, cams = traj._scene(71, N, W, H, 0.06)
    # no row near min_opacity = 0.005 (raw -5.29): ten Adam steps move a raw opacity by well under 1, so both loops agree on
    # which rows are dead; every seventh row at o = 0.018, where the noise's gate is open (0.21)
    p0["opacity"] = np.maximum(p0["opacity"], np.float32(-4.0))
    p0["opacity"][::7] = np.float32(-4.0)
    return p0, cams


def _bars(got, want, p0, report, tag="param"):
    traj._compare(tag, got, want, p0, report)


def test_fused_step_matches_unfused_and_numpy(oracle32):
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    from gaussiansplattingmlx_amd.scenes import perturb
    _gpu()
    W, H = 160, 120
    p0, cams = _scene_with_dim_rows()
    target = oracle32.render_forward(perturb(p0, 5, 0.1), cams[0].as_dict(), W, H, 16, 16, 4)["color"].reshape(H, W, 3).copy()
    cfg = MCMCConfig(cap_max=4000, refine_start=10**6)
    states = {}
    for fused in (True, False):
        r = _renderer(W, H)
        tr, model = _mcmc_trainer(r, p0, cfg, fuse_adam=fused)
        tr.trainStep(cams[0], torch.as_tensor(target, device="cuda"), viewKey=0)
        states[fused] = _state(model)
    p = {k: v.copy() for k, v in p0.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    _numpy_step(oracle32, p, m, v, cams[0], target, W, H, 0, cfg, tr.noise_seed)
    report = {}
    _bars(states[True][0], states[False][0], p0, report, "fused_vs_unfused")
    _bars(states[True][0], p, p0, report, "fused_vs_numpy")
    _bars(states[True][1], m, p0, report, "m")
    moved = np.abs(states[True][0]["xyz"][::7] - p0["xyz"][::7]).max()
    assert moved > 1e-3, moved          # the noise moved the dim rows
    for k in KEYS:
        for tag in ("fused_vs_unfused", "fused_vs_numpy", "m"):
            e = report[f"{tag}.{k}"]
            assert e["share_beyond"] <= traj.MOMENT_SHARE and e["max_rel"] <= 2e-2, (tag, k, e)


# ---------------------------------------------------------------------------------------------------------- the event
def _event_scene(N=4000, K=16, seed=11):
    p = _rows(seed, N, K)
    rng = np.random.default_rng(seed + 1)
    dead = np.sort(rng.choice(N, 600, replace=False))
    p["opacity"][dead] = rng.uniform(-14, -6, dead.size).astype(np.float32)
    p["opacity"][dead[:3]] = [np.nan, np.inf, -np.inf]
    live = np.setdiff1d(np.arange(N), dead)
    p["opacity"][live] = rng.uniform(-4, 3, live.size).astype(np.float32)
    p["opacity"][live[:5]] = 6.0                  # a few dominant weights
    return p


def _arena(p, capacity=None):
    from gaussiansplattingmlx_amd.trainer import GaussModel
    m = GaussModel(p, torch.device("cuda"))
    m.restride(capacity or m.N)
    rng = np.random.default_rng(5)
    m.m.copy_(torch.as_tensor(rng.normal(0, 1, m.m.numel()).astype(np.float32)))
    m.v.copy_(torch.as_tensor(rng.uniform(0, 1, m.v.numel()).astype(np.float32)))
    return m


def test_relocation_on_a_crafted_scene():
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig, relocation_formula
    _gpu()
    r = _renderer()
    p = _event_scene()
    cfg = MCMCConfig()
    t, seed = 600, 20260313
    prm = cfg.params(t, seed)
    # before the device runs: no draw's target is within 1e-9 of the total from a prefix entry (the device's prefix differs
    # from numpy's by its summation order, about N 2^-53), so every draw has one possible source and none is excused
    src, target, cdf, rows, dead = mn.draw(p["opacity"], 0, cfg.min_opacity, 600, seed, t)
    assert mn.min_boundary_gap(cdf, target) >= 1e-9
    outs = []
    for _ in range(2):
        model = _arena(p)
        before = _state(model)
        st = r.mcmcRelocate(model.getParams(), model.arena, model.m, model.v, prm)
        outs.append((_state(model), st))
    (got, gm, gv), st = outs[0]
    for a, b in zip(outs[0][0], outs[1][0]):
        for k in KEYS:
            assert np.array_equal(a[k], b[k], equal_nan=True), k           # deterministic, bit for bit
    assert st["dead"] == dead.size == 600 and st["relocated"] == 600 and st["live"] == rows.size
    o = mn.sigmoid(got["opacity"])
    assert np.isfinite(got["opacity"]).all() and (o > cfg.min_opacity).all()               # no dead row is left
    # every destination is a copy of the restated sampler's source, a live row
    fp = lambda s, i: np.concatenate([s[k][i].reshape(-1) for k in KEYS])                # noqa: E731
    for j, i in enumerate(dead):
        assert np.array_equal(fp(got, src[j]), fp(got, i)), j
    hip_src = src
    assert (mn.sigmoid(p["opacity"][hip_src]) > cfg.min_opacity).all()
    # opacity and scale of the sources: the float64 formula
    cnt = np.bincount(hip_src, minlength=p["opacity"].size)
    s_rows = np.nonzero(cnt)[0]
    on, ratio = relocation_formula(mn.sigmoid(p["opacity"][s_rows]), cnt[s_rows] + 1, cfg.min_opacity, cfg.n_max)
    np.testing.assert_allclose(mn.sigmoid(got["opacity"][s_rows]), on, rtol=1e-6)
    np.testing.assert_allclose(np.exp(got["scales"][s_rows].astype(np.float64)),
                               np.exp(p["scales"][s_rows].astype(np.float64)) * ratio[:, None], rtol=1e-6)
    # moments zero on touched rows; every other row and moment bit for bit
    touched = np.zeros(p["opacity"].size, bool)
    touched[dead] = touched[s_rows] = True
    for k in KEYS:
        assert (gm[k][touched] == 0).all() and (gv[k][touched] == 0).all(), k
        assert np.array_equal(gm[k][~touched], before[1][k][~touched]) and np.array_equal(gv[k][~touched], before[2][k][~touched])
        assert np.array_equal(got[k][~touched], before[0][k][~touched], equal_nan=True), k


def test_growth():
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig, relocation_formula
    _gpu()
    r = _renderer()
    p = _event_scene()
    N = p["opacity"].size
    cfg = MCMCConfig(cap_max=int(N * 1.2))
    src, target, cdf, rows, _ = mn.draw(p["opacity"], 1, cfg.min_opacity, 200, 3, 700)
    assert mn.min_boundary_gap(cdf, target) >= 1e-9      # (before the device runs: every draw has one possible source)
    model = _arena(p, cfg.cap_max)
    ptr = model.arena.data_ptr()
    want = mn.event(*_state(model), 1, cfg, 700, 3)
    N1 = r.mcmcGrow(model.getParams(), model.stride, model.arena, model.m, model.v, cfg.params(700, 3))
    assert N1 == min(cfg.cap_max, int(1.05 * N)) == 4200 == want["N"]
    model.setCount(N1)
    assert model.arena.data_ptr() == ptr
    got, gm, gv = _state(model)
    assert np.array_equal(want["sources"], src)
    cnt = np.bincount(src, minlength=N)
    s_rows = np.nonzero(cnt)[0]
    on, ratio = relocation_formula(mn.sigmoid(p["opacity"][s_rows]), cnt[s_rows] + 1, cfg.min_opacity, cfg.n_max)
    np.testing.assert_allclose(mn.sigmoid(got["opacity"][s_rows]), on, rtol=1e-6)
    for k in KEYS:
        assert (gm[k][N:] == 0).all() and (gv[k][N:] == 0).all()
    # the appended rows are copies of the modified sources, every draw's source the restatement's; what the event does not
    # modify is the restatement's bit for bit
    for k in KEYS:
        assert np.array_equal(got[k][N:], got[k][src]), k
        if k not in ("opacity", "scales"):
            assert np.array_equal(got[k], want["p"][k]), k
        assert np.array_equal(gm[k], want["m"][k]) and np.array_equal(gv[k], want["v"][k]), k
    quiet = np.setdiff1d(np.arange(N), s_rows)
    assert np.array_equal(got["opacity"][quiet], want["p"]["opacity"][quiet], equal_nan=True)
    assert np.array_equal(got["scales"][quiet], want["p"]["scales"][quiet])
    # at the cap: nothing added; the edge cases do not raise
    assert r.mcmcGrow(model.getParams(), model.stride, model.arena, model.m, model.v,
                      MCMCConfig(cap_max=N1).params(800, 3)) == N1
    for fill in (-20.0, 3.0, np.nan):
        q = {k: v.copy() for k, v in p.items()}
        q["opacity"][:] = fill
        mm = _arena(q, int(N * 1.2))
        st = r.mcmcRelocate(mm.getParams(), mm.arena, mm.m, mm.v, cfg.params(900, 3))
        assert st["relocated"] == 0
        n2 = r.mcmcGrow(mm.getParams(), mm.stride, mm.arena, mm.m, mm.v, cfg.params(900, 3))
        assert n2 == (N if np.isnan(fill) else 4200), (fill, n2)


# ---------------------------------------------------------------------------------------------------------- trainers
def test_default_non_interference():
    """strategy='mcmc' with zero regularisers, zero noise and no event in the window against a densify=False default trainer
    over ten steps.  The terms add +0.0 and the strided layout changes no value a kernel computes, but the blend backward sums a
    splat's per-pixel terms with float atomics, so two DEFAULT trainers already part after the first update (DESIGN.md section
    11).  So: bit for bit where the two default runs agree bit for bit, else the first loss bit for bit (the forward of the
    same start) and every later one, the parameters and the moments within test_gpu_trajectory's bars against the spread of
    the two default runs."""
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer, GaussModel
    _gpu()
    W, H = 160, 120
    p0, cams = traj._scene(71, 3000, W, H, 0.06)
    tp = perturb(p0, 5, 0.1)
    from oracle.oracle import Oracle
    o = Oracle(np.float32)
    targets = [torch.as_tensor(o.render_forward(tp, c.as_dict(), W, H, 16, 16, 4)["color"].reshape(H, W, 3).copy(), device="cuda")
               for c in cams]
    out = []
    for mc in (False, False, True):
        r = _renderer(W, H)
        model = GaussModel(p0, r.device)
        kw = dict(strategy="mcmc", mcmc=MCMCConfig(cap_max=5000, noise_lr=0.0, opacity_reg=0.0, scale_reg=0.0,
                                                     refine_start=10**6)) if mc else dict(densify=False)
        tr = GaussianTrainer(model, r, iterationCount=traj.TOTAL, **kw)
        losses = [float(tr.trainStep(cams[i % 3], targets[i % 3], viewKey=i % 3)[0]) for i in range(10)]
        out.append((losses, _state(model)))
    (la, sa), (lb, sb), (lc, sc) = out
    same = la == lb and all(np.array_equal(x[k], y[k]) for x, y in zip(sa, sb) for k in KEYS)
    if same:
        assert lc == la
        for a, c in zip(sa, sc):
            for k in KEYS:
                assert np.array_equal(a[k], c[k]), k
        return
    assert lc[0] == la[0] == lb[0]
    assert np.abs(np.asarray(lc) - np.asarray(la)).max() <= traj.LOSS_TOL
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, getLearningRates
    lr = dict(zip(PARAM_ORDER, getLearningRates(0, traj.TOTAL)))
    report = {}
    for i, tag in enumerate(("param", "m", "v")):
        traj._compare(tag, sc[i], sa[i], p0, report)
        traj._compare("default." + tag, sb[i], sa[i], p0, report)
    for k in KEYS:
        for tag in ("m", "v"):
            e = report[f"{tag}.{k}"]
            assert e["share_beyond"] <= traj.MOMENT_SHARE and e["max_rel"] <= 2e-2, (tag, k, e)
        e, ref = report[f"param.{k}"], report[f"default.param.{k}"]
        assert e["share_beyond"] <= 1.5 * ref["share_beyond"] + 5e-4, (k, e, ref)
        assert e["max_abs"] <= 2 * 3.17 * lr[k] * 10 * 1.01 + 1e-6, (k, e)


def test_trajectory_with_an_event(oracle32):
    """Ten fused MCMC steps, the event behind the last one, against the oracle loop with the numpy regularisers, noise and
    event: every step's loss and the rows neither event touched within test_gpu_trajectory's bars; the same dead rows refilled,
    the same count grown, every refilled or appended row a copy of a row the device kept."""
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig, grown_count
    from gaussiansplattingmlx_amd.scenes import perturb
    from gaussiansplattingmlx_amd.trainer import PARAM_ORDER, getLearningRates
    _gpu()
    W, H, STEPS = 160, 120, traj.STEPS
    p0, cams = _scene_with_dim_rows()
    p0["opacity"][3::11] = np.float32(-11.0)          # dead from the start (o = 1.7e-5), no gradient can revive them in 10 steps
    N = p0["opacity"].size
    tp = perturb(p0, 5, 0.1)
    targets = [oracle32.render_forward(tp, c.as_dict(), W, H, 16, 16, 4)["color"].reshape(H, W, 3).copy() for c in cams]
    cfg = MCMCConfig(cap_max=int(N * 1.2), refine_start=STEPS - 2, refine_stop=STEPS, refine_every=STEPS - 1)
    r = _renderer(W, H)
    tr, model = _mcmc_trainer(r, p0, cfg)
    tg = [torch.as_tensor(t, device="cuda") for t in targets]
    got_l = [float(tr.trainStep(cams[i % 3], tg[i % 3], viewKey=i % 3)[0]) for i in range(STEPS)]
    gp, gm, _ = _state(model)
    st = tr.lastMCMCStats
    p = {k: v.copy() for k, v in p0.items()}
    m = {k: np.zeros_like(v) for k, v in p.items()}
    v = {k: np.zeros_like(x) for k, x in p.items()}
    want_l = [_numpy_step(oracle32, p, m, v, cams[i % 3], targets[i % 3], W, H, i, cfg, tr.noise_seed) for i in range(STEPS)]
    dl = np.abs(np.asarray(got_l) - np.asarray(want_l))
    assert dl.max() <= traj.LOSS_TOL and got_l[-1] < got_l[0], (dl.tolist(), got_l, want_l)
    _, _, _, _, dead = mn.draw(p["opacity"], 0, cfg.min_opacity, 1, tr.noise_seed, STEPS - 1)
    assert st["dead"] == dead.size and st["relocated"] == dead.size and st["N"] == grown_count(N, cfg.cap_max, cfg.grow_rate)
    assert model.N == st["N"] and st["added"] == st["N"] - N
    touched_dev = np.all(np.concatenate([gm[k][:N].reshape(N, -1) for k in KEYS], 1) == 0, 1)    # sources + destinations
    assert touched_dev[dead].all()
    keep = ~touched_dev
    keep[dead] = False
    report = {}
    traj._compare("param", {k: gp[k][:N][keep] for k in KEYS}, {k: p[k][keep] for k in KEYS}, p0, report)
    lr = dict(zip(PARAM_ORDER, getLearningRates(0, traj.TOTAL)))
    for k in KEYS:
        e = report[f"param.{k}"]
        assert e["share_beyond"] <= 0.01 and e["max_abs"] <= 2 * 3.17 * lr[k] * STEPS * 1.01 + 0.5 * (k == "xyz"), (k, e)
    # (position, colour and rotation: a source drawn by both the relocation and the growth has its opacity and scale
    # modified twice, the relocation's copies hold the first modification)
    rowsig = lambda i: np.concatenate([gp[k][i].reshape(-1) for k in ("xyz", "features_dc", "features_rest", "rotation")]).tobytes()  # noqa: E731
    kept = {rowsig(i) for i in np.nonzero(touched_dev)[0] if i not in set(dead.tolist())}
    for i in list(dead) + list(range(N, model.N)):
        assert rowsig(i) in kept, i


def test_short_aa_run_with_growth_stays_in_budget():
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    from gaussiansplattingmlx_amd.scenes import perturb
    _gpu()
    W = H = 400
    p0, _ = traj._scene(17, 10_000, W, H, 0.03)
    cams = [Camera(W, H, 0.9 * W, 0.9 * W, look_at_c2w(e)) for e in ([2.2, -2.6, 1.7], [-2.9, 1.4, 1.2], [0.6, 3.1, 2.0])]
    r = _renderer(W, H, aa=True)
    tp = perturb(p0, 5, 0.1)
    targets = []
    for c in cams:
        res = r.renderForward({k: torch.as_tensor(v, device="cuda") for k, v in tp.items()}, c)
        targets.append(res.render.clone())
    cap = int(1.2 * 10_000)
    cfg = MCMCConfig(cap_max=cap, refine_start=0, refine_every=5, refine_stop=40)
    tr, model = _mcmc_trainer(r, p0, cfg)
    losses = []
    for i in range(40):
        losses.append(float(tr.trainStep(cams[i % 3], targets[i % 3], viewKey=i % 3)[0]))
        assert model.N <= cap
    assert model.N == cap and np.isfinite(losses).all()
    for k in KEYS:
        assert torch.isfinite(model.getParams()[k]).all(), k
    assert np.mean(losses[-6:]) < np.mean(losses[:6]), losses
