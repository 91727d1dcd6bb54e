"""Sparse Adam without a device (gaussiansplattingmlx_amd/sparse_adam.py, include/gsplat.h gs_set_sparse_adam, DESIGN.md section
17): the numpy float32 statement of the rule, the element -> row map of a GaussModel layout against brute force, the visible
counts of the scenes the GPU tests use from both oracles, the trainer's refusals and the entry points' declaration.

Scenes: test_gpu_trajectory._scene(71, N, 160, 120, 0.06), its K = 25 rows cut to the case's K.  Camera A is that scene's camera
0 and sees every Gaussian; camera B, Camera(160, 120, 144, 144 * 1.02, look_at_c2w([0.4, -0.5, 0.3])), stands inside the cloud.
"""
import importlib.util
import os
import re

import numpy as np
import pytest

from gaussiansplattingmlx_amd import sparse_adam as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ("gs_set_sparse_adam", "gs_get_visibility", "gs_adam_step_visible")
W, H = 160, 120
# (N, K): visible, invisible from camera B
TABLE = {(3000, 25): (2436, 564), (3001, 25): (2437, 564), (1500, 16): (1214, 286), (700, 4): (572, 128), (333, 1): (276, 57)}
DEGREE = {25: 4, 16: 3, 4: 1, 1: 0}
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")


def _load(name):
    spec = importlib.util.spec_from_file_location("_sa_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_cache = {}


def scene(N, K=25):
    """(params with K SH coefficients, [camera A, camera B, camera C])."""
    if (N, K) not in _cache:
        from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
        p, cams = _load("test_gpu_trajectory")._scene(71, N, W, H, 0.06)
        p = dict(p)
        p["features_rest"] = np.ascontiguousarray(p["features_rest"][:, :K - 1])
        inside = [Camera(W, H, 144, 144 * 1.02, look_at_c2w(eye)) for eye in ([0.4, -0.5, 0.3], [-0.5, 0.3, 0.35])]
        _cache[(N, K)] = (p, [cams[0]] + inside)
    return _cache[(N, K)]


def oracle_visible(o, N, K, cam):
    """radii > 0 of the oracle's projection of scene (N, K) from `cam`."""
    key = ("vis", np.dtype(o.dtype).name, N, K, id(cam))
    if key not in _cache:
        p, _ = scene(N, K)
        _, sc, rt = o.activations_forward(p["opacity"], p["scales"], p["rotation"])
        shs = np.concatenate([p["features_dc"], p["features_rest"]], axis=1)
        c = cam.as_dict()
        pr = o.projection_forward(sc, rt, p["xyz"], shs, c["camCenter"], c["view"], c["proj"], c["fovX"], c["fovY"], c["focalX"],
                                  c["focalY"], W, H, DEGREE[K])
        vis = np.asarray(pr["radii"]).reshape(-1) > 0
        vis.setflags(write=False)
        _cache[key] = vis
    return _cache[key]


def blocked_order(vis):
    """The permutation that puts the invisible rows first (stable within each group)."""
    return np.concatenate([np.flatnonzero(~vis), np.flatnonzero(vis)])


# ------------------------------------------------------------------------------------------------------------ the numpy rule
def _state(n, seed):
    rng = np.random.default_rng(seed)
    p, g = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    m, v = (0.1 * rng.normal(size=n)).astype(np.float32), (0.01 * rng.random(n)).astype(np.float32)
    return p, g, m, v


def test_all_ones_mask_is_dense_adam_bit_for_bit():
    n = 1003
    p, g, m, v = _state(n, 1)
    lr = np.float32(1.6e-4)
    # dense numpy Adam, written out as test_adam_step_matches_numpy writes it
    one = np.float32(1)
    b1, b2, eps = np.float32(0.9), np.float32(0.999), np.float32(1e-15)
    m2 = b1 * m + (one - b1) * g
    v2 = b2 * v + (one - b2) * g * g
    p2 = p - lr * m2 / (np.sqrt(v2) + eps)
    got = sa.adam_visible(p, g, m, v, lr, np.ones(n, bool))
    for a, b in zip(got, (p2, m2, v2)):
        assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    d = sa.adam_dense(p, g, m, v, lr)
    for a, b in zip(got, d):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_masked_rows_come_back_bit_for_bit():
    N, width = 257, 7
    p, g, m, v = (a.reshape(N, width) for a in _state(N * width, 2))
    p[3, 2] = np.float32("nan")                 # (whatever bits an invisible row holds)
    m[5, 0] = np.float32(-0.0)
    vis = np.random.default_rng(3).random(N) < 0.4
    vis[3] = vis[5] = False
    p2, m2, v2 = sa.adam_visible_rows(p, g, m, v, 1e-3, vis)
    for a, b in ((p2, p), (m2, m), (v2, v)):
        assert np.array_equal(a[~vis].view(np.uint32), b[~vis].view(np.uint32))
    dp, dm, dv = sa.adam_dense(p, g, m, v, 1e-3)
    for a, b in ((p2, dp), (m2, dm), (v2, dv)):
        assert np.array_equal(a[vis].view(np.uint32), b[vis].view(np.uint32))
    assert (p2[vis] != p[vis]).all() and (m2[vis] != m[vis]).all()


def test_three_rows_by_hand():
    # row 0: visible, g = 1; row 1: invisible, g = 1 (ignored); row 2: visible, g = 0 -- its moments decay, it still moves
    p = np.array([[1.0], [2.0], [3.0]], np.float32)
    g = np.array([[1.0], [1.0], [0.0]], np.float32)
    m = np.array([[0.0], [0.5], [0.5]], np.float32)
    v = np.array([[0.0], [0.25], [0.25]], np.float32)
    p2, m2, v2 = sa.adam_visible_rows(p, g, m, v, np.float32(0.1), [1, 0, 1])
    f = np.float32
    one = f(1)
    # row 0: m = 0.1 (as float32 forms 1 - 0.9), v = 0.001 (likewise), step = 0.1 * m / sqrt(v)
    m0, v0 = (one - f(0.9)) * one, (one - f(0.999)) * one
    assert m2[0, 0] == m0 and v2[0, 0] == v0
    assert m2[0, 0] == f(0.100000024) and v2[0, 0] == f(0.0009999871)
    assert p2[0, 0] == f(1.0) - f(0.1) * m0 / (np.sqrt(v0) + f(1e-15))
    assert abs(float(p2[0, 0]) - (1.0 - 0.1 * 0.1 / np.sqrt(0.001))) < 1e-5
    # row 1: every bit as it was
    assert (p2[1, 0], m2[1, 0], v2[1, 0]) == (f(2.0), f(0.5), f(0.25))
    # row 2: m = 0.9 * 0.5 = 0.45, v = 0.999 * 0.25 = 0.24975, p = 3 - 0.1 * 0.45 / sqrt(0.24975)
    assert m2[2, 0] == f(0.9) * f(0.5) and v2[2, 0] == f(0.999) * f(0.25)
    assert m2[2, 0] == f(0.45) and v2[2, 0] == f(0.24975)
    assert abs(float(p2[2, 0]) - (3.0 - 0.1 * 0.45 / np.sqrt(0.24975))) < 1e-6
    assert p2[2, 0] < p[2, 0]


# ------------------------------------------------------------------------------------------------------ element -> row map
def _brute_rows(model):
    """Row of every element, by walking every tensor's segment element by element."""
    from gaussiansplattingmlx_amd.trainer import ARENA_ORDER
    rows = np.full(model.numel, -1, np.int64)
    starts = [0] + [int(x) for x in model.seg_end[:-1]]
    for k, s0, s1 in zip(ARENA_ORDER, starts, model.seg_end):
        per = max(model._per[k], 1)
        for e in range(s0, int(s1)):
            rows[e] = (e - s0) // per
    return rows


@pytest.mark.parametrize("N,K,capacity", [(7, 4, None), (9, 1, None), (5, 25, None), (7, 4, 12), (1, 16, 3), (6, 25, 6)])
def test_element_rows_match_brute_force(N, K, capacity):
    import torch
    from gaussiansplattingmlx_amd.trainer import ARENA_ORDER, GaussModel
    rng = np.random.default_rng(N)
    p = dict(xyz=rng.normal(size=(N, 3)), features_dc=rng.normal(size=(N, 1, 3)), features_rest=rng.normal(size=(N, K - 1, 3)),
             scales=rng.normal(size=(N, 3)), rotation=rng.normal(size=(N, 4)), opacity=rng.normal(size=N))
    model = GaussModel({k: torch.as_tensor(np.ascontiguousarray(v, np.float32)) for k, v in p.items()}, "cpu")
    if capacity is not None:
        model.restride(capacity)
        assert model.stride == capacity
    widths = sa.model_row_floats(model)
    assert widths == [3, 3, 4, 1, 3, max(3 * (K - 1), 1)]
    rows = sa.model_element_rows(model)
    assert np.array_equal(rows, _brute_rows(model))
    # every element of a Gaussian's row in every tensor maps to that Gaussian; everything else to a row >= N
    marked = np.zeros(model.numel, bool)
    model.arena.zero_()
    for k, view in model.getParams().items():
        for r in range(N):
            view[r] = 1.0
            on = model.arena.numpy() != 0
            assert (rows[on] == r).all() and int(on.sum()) == model._per[k], (k, r)
            marked |= on
            view[r] = 0.0
    assert (rows[~marked] >= N).all() and (rows[marked] < N).all()
    assert int(marked.sum()) == N * model.floats_per_gaussian
    # the element mask of a row mask
    vis = rng.random(N) < 0.5
    on = sa.element_mask(vis, model.seg_end, widths, N)
    assert int(on.sum()) == int(vis.sum()) * model.floats_per_gaussian and not on[~marked].any()
    assert list(ARENA_ORDER) == ["xyz", "scales", "rotation", "opacity", "features_dc", "features_rest"]


def test_element_rows_refuses_bad_layouts():
    with pytest.raises(ValueError):
        sa.element_rows([4, 8], [3])
    with pytest.raises(ValueError):
        sa.element_rows([4, 8], [3, 0])
    with pytest.raises(ValueError):
        sa.element_rows([8, 4], [3, 3])
    with pytest.raises(ValueError):
        sa.element_rows([4, 8], [3, 3], n=9)


# ----------------------------------------------------------------------------------------------------- the scenes' counts
@pytest.mark.parametrize("N,K", sorted(TABLE))
def test_visible_counts_of_the_scenes(oracle32, oracle64, N, K):
    _, cams = scene(N, K)
    a32, a64 = oracle_visible(oracle32, N, K, cams[0]), oracle_visible(oracle64, N, K, cams[0])
    assert a32.all() and a64.all()                                  # camera A sees every Gaussian
    b32, b64 = oracle_visible(oracle32, N, K, cams[1]), oracle_visible(oracle64, N, K, cams[1])
    assert np.array_equal(b32, b64)                                 # no borderline case: the device mask must equal it exactly
    assert (int(b32.sum()), int((~b32).sum())) == TABLE[(N, K)]


def test_row_orders_of_the_large_scene(oracle32):
    _, cams = scene(3000, 25)
    vis = oracle_visible(oracle32, 3000, 25, cams[1])
    # scattered (the natural order): every one of the 46 full waves of 64 rows is mixed
    full = vis[:46 * 64].reshape(46, 64).sum(axis=1)
    assert ((full > 0) & (full < 64)).all()
    # blocked: the invisible rows first -- four all-invisible workgroups of 128 rows, then wave 8 mixed at 52 / 12
    order = blocked_order(vis)
    b = vis[order]
    assert not b[:512].any() and not b[:564].any() and b[564:].all()
    assert (int((~b[512:576]).sum()), int(b[512:576].sum())) == (52, 12)


# ------------------------------------------------------------------------------------------------------------- the trainer
@pytest.mark.parametrize("kw", [dict(process_group=object()), dict(dp_bootstrap=(b"", 0, 1)), dict(exchange_impl="native"),
                                dict(views_per_rank=2), dict(strategy="mcmc"), dict(filter_3d=True), dict(sparse_adam=1),
                                dict(sparse_adam="yes"), dict(sparse_adam=None)])
def test_trainer_refuses(kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(sparse_adam=True)
    args.update(kw)
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


# ------------------------------------------------------------------------------------------------------------ entry points
def test_header_and_binding_declare_the_entries():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from gaussiansplattingmlx_amd import _lib
    for e in ENTRIES:
        assert re.search(r"\bint " + e + r"\s*\(", plain), e
        assert e in _lib.exported_symbols()
        assert e in _lib._SIGS
    assert "radius > 0" in src and "bit for bit" in src        # the header states the rule


def test_null_context_is_refused():
    from gaussiansplattingmlx_amd import build, _lib
    build.build()
    lib = _lib.load()
    assert lib.gs_set_sparse_adam(None, 1) == 1
    assert lib.gs_get_visibility(None, 0, None) == 1
    assert lib.gs_adam_step_visible(None, 0, None, None, None, None, 1, None, None, None, 0.9, 0.999, 1e-15, 1.0, 0, None) == 1
