"""Mesh extraction on the device (include/gsplat.h gs_tsdf_*, gaussiansplattingmlx_amd/mesh.py) against
the float32 restatement (tests/tsdf_numpy.py), BIT FOR BIT: csrc/tsdf.hip is compiled without contraction and the restatement
follows its written order, so every volume word, every vertex, colour and face index is compared as an integer.  The float64
restatement bounds the float32 one as in tests/test_tsdf_cpu.py (1e-5 where the pixel and truncation decisions agree).

Shapes: 20 x 17 x 13 (non-cubic, no dimension a multiple of 64: an index-order or tail bug shows), 2 x 2 x 2 (one cell), the
12^3 / 9^3 analytic grids, 65^3 = 274625 lattice points = 269 scan tiles (more than the TSDF_THREADS = 256 tiles one pass of
the top-level scan handles: its carry) and 16 x 16 x 8 = 2048 = exactly two scan tiles of TSDF_SCAN_TILE = 1024.

Measured (MI355X): every bitwise comparison holds; the integrated volume is within 6.7e-7 (tsdf) and 6e-8 (colour) of the float64
restatement, no voxel's decisions differ; the end-to-end mesh has 40744 vertices and 81088 triangles; the file runs in 3 s."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TSDF_THREADS, TSDF_SCAN_TILE = 256, 1024        # csrc/tsdf.hip


def _load(name):
    spec = importlib.util.spec_from_file_location("_tsdfg_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tn = _load("tsdf_numpy")
_shared = {}


@pytest.fixture(scope="module")
def r():
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    ren = GaussianRenderer(4, 128, 128, (16, 16), False)
    yield ren
    _shared.clear()
    ren.close()


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0]}"


def _grid_struct(grid):
    from gaussiansplattingmlx_amd import _lib
    g = _lib.gs_tsdf_grid()
    for i in range(3):
        g.origin[i] = float(grid["origin"][i])
    g.voxel, g.trunc = float(grid["voxel"]), float(grid["trunc"])
    g.nx, g.ny, g.nz = grid["dims"]
    return g


def _view_structs(views):
    """(ctypes array, the device tensors it points to)"""
    from gaussiansplattingmlx_amd import _lib
    arr = (_lib.gs_tsdf_view * max(len(views), 1))()
    held = []
    for k, vw in enumerate(views):
        for i, x in enumerate(np.asarray(vw["Rt"], np.float32).reshape(12)):
            arr[k].Rt[i] = float(x)
        arr[k].fx, arr[k].fy, arr[k].cx, arr[k].cy = (float(vw[q]) for q in ("fx", "fy", "cx", "cy"))
        arr[k].height, arr[k].width = vw["depth"].shape
        d = _dev(vw["depth"])
        c = None if vw.get("color") is None else _dev(vw["color"])
        held.append((d, c))
        arr[k].depth, arr[k].color = d.data_ptr(), (None if c is None else c.data_ptr())
    return arr, held


def _dev_volume(vol):
    return {k: (None if v is None else _dev(v)) for k, v in vol.items()}


def _integrate(r, grid, views, dv, batch):
    """gs_tsdf_integrate over `views` in calls of `batch`; the last status."""
    g = _grid_struct(grid)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    rc = 0
    for at in range(0, len(views), batch):
        arr, held = _view_structs(views[at:at + batch])
        rc = r.lib.gs_tsdf_integrate(r.ctx, C.byref(g), len(views[at:at + batch]), arr, p(dv["tsdf"]), p(dv["weight"]), p(dv["rgb"]),
                                     p(dv["cweight"]))
        r.sync()
        if rc:
            break
    return rc


def _scene():
    """The integrate scene with both restatements, computed once and never written."""
    if "scene" not in _shared:
        grid, views = tn.integrate_scene(3)
        d32 = []
        v32 = tn.integrate(grid, views, tn.empty_volume(grid), np.float32, d32)
        d64 = []
        v64 = tn.integrate(grid, views, tn.empty_volume(grid, dtype=np.float64), np.float64, d64)
        agree = np.ones(v32["tsdf"].shape, bool)
        for a, b in zip(d32, d64):
            for x, y in zip(a, b):
                agree &= x == y
        _shared["scene"] = (grid, views, v32, v64, agree)
    return _shared["scene"]


def test_integrate_equals_the_float32_restatement_bit_for_bit(r):
    grid, views, v32, v64, agree = _scene()
    assert grid["dims"] == (20, 17, 13) and all(v["depth"].shape == (80, 96) for v in views)
    assert np.isnan(views[0]["depth"]).sum() == 1 and (views[0]["depth"][30:40, 40:52] == 0).all()
    dv = _dev_volume(tn.empty_volume(grid))
    assert _integrate(r, grid, views, dv, 8) == 0
    for k in ("tsdf", "weight", "rgb", "cweight"):
        _same_bits(_np(dv[k]), v32[k], k)
        err = float(np.abs(_np(dv[k])[agree].astype(np.float64) - v64[k][agree]).max())
        print(k, "against float64", err)
        assert err <= 1e-5
    assert 1.0 - agree.mean() <= 0.005
    # without the colour pair: the same tsdf and weight
    dn = _dev_volume(tn.empty_volume(grid, color=False))
    assert _integrate(r, grid, views, dn, 8) == 0
    _same_bits(_np(dn["tsdf"]), v32["tsdf"], "tsdf without colour")
    _same_bits(_np(dn["weight"]), v32["weight"], "weight without colour")


def test_batches_of_views_equal_one_view_calls(r):
    grid, views = tn.integrate_scene(11)
    a, b = _dev_volume(tn.empty_volume(grid)), _dev_volume(tn.empty_volume(grid))
    assert _integrate(r, grid, views, a, 8) == 0           # 8 + 3
    assert _integrate(r, grid, views, b, 1) == 0           # 11 x 1
    want = tn.integrate(grid, views, tn.empty_volume(grid))
    for k in a:
        _same_bits(_np(a[k]), _np(b[k]), k + " (8 + 3 against 11 x 1)")
        _same_bits(_np(a[k]), want[k], k)
    assert float(_np(a["weight"]).max()) >= 4
    before = {k: _np(v).copy() for k, v in a.items()}
    g = _grid_struct(grid)
    arr, held = _view_structs(views[:9])
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for n_views in (9, 0, -1):
        assert r.lib.gs_tsdf_integrate(r.ctx, C.byref(g), n_views, arr, p(a["tsdf"]), p(a["weight"]), p(a["rgb"]), p(a["cweight"])) == 1
    assert r.lib.gs_tsdf_integrate(r.ctx, C.byref(g), 1, arr, p(a["tsdf"]), p(a["weight"]), p(a["rgb"]), None) == 1
    arr[0].depth = None
    assert r.lib.gs_tsdf_integrate(r.ctx, C.byref(g), 1, arr, p(a["tsdf"]), p(a["weight"]), p(a["rgb"]), p(a["cweight"])) == 1
    r.sync()
    for k in a:
        _same_bits(_np(a[k]), before[k], k + " after refused calls")


def test_views_that_see_nothing_leave_every_bit(r):
    grid, views, v32, _, _ = _scene()
    start = {k: v.copy() for k, v in v32.items()}
    start["tsdf"][5] = np.float32(np.nan)                  # (a payload a rewritten word could lose)
    start["tsdf"].view(np.int32)[6] = 0x7FC12345
    dv = _dev_volume(start)
    W, H = 96, 80
    full = np.full((H, W), 1.5, np.float32)
    col = np.full((H, W, 3), 0.25, np.float32)
    behind = dict(Rt=tn.look_at_Rt((3.0, 0.5, 0.4), target=(6.0, 1.0, 0.8)), fx=100.0, fy=100.0, cx=48.0, cy=40.0, depth=full, color=col)
    aside = dict(Rt=tn.look_at_Rt((3.0, 0.5, 0.4), target=(3.0, 30.0, 0.4)), fx=400.0, fy=400.0, cx=48.0, cy=40.0, depth=full, color=col)
    for vw in (behind, aside):          # (the cases are what they claim: the restatement changes nothing either)
        chk = {k: v.copy() for k, v in start.items()}
        dec = []
        tn.integrate(grid, [vw], chk, np.float32, dec)
        assert (dec[0][0] == -1).all()
    p = tn.lattice_points(grid, np.float64)
    assert ((p @ behind["Rt"][:, :3].T.astype(np.float64) + behind["Rt"][:, 3])[:, 2] < 0).all()
    assert ((p @ aside["Rt"][:, :3].T.astype(np.float64) + aside["Rt"][:, 3])[:, 2] > 0).any()
    assert _integrate(r, grid, [behind, aside], dv, 8) == 0
    for k in dv:
        _same_bits(_np(dv[k]), start[k], k)


def _extract(r, grid, tsdf, weight, min_weight, rgb=None, cweight=None):
    """plan + emit through the C ABI: (vertices, faces, colors, (V, F)) as numpy."""
    g = _grid_struct(grid)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    t = [None if x is None else _dev(x) for x in (tsdf, weight, rgb, cweight)]
    nbytes = int(r.lib.gs_tsdf_mesh_workspace_bytes(C.byref(g)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    counts = (C.c_longlong * 2)()
    r._check(r.lib.gs_tsdf_mesh_plan(r.ctx, C.byref(g), p(t[0]), p(t[1]), C.c_float(min_weight), p(ws), nbytes, counts))
    V, F = int(counts[0]), int(counts[1])
    # one row more than planned, NaN / -7 filled: everything planned is written, nothing beyond
    vert = torch.full((V + 1, 3), float("nan"), device="cuda")
    cols = torch.full((V + 1, 3), float("nan"), device="cuda") if rgb is not None else None
    faces = torch.full((F + 1, 3), -7, dtype=torch.int32, device="cuda")
    r._check(r.lib.gs_tsdf_mesh_emit(r.ctx, C.byref(g), p(t[0]), p(t[1]), p(t[2]), p(t[3]), C.c_float(min_weight), p(ws), p(vert),
                                     p(cols), p(faces)))
    r.sync()
    vert, faces = _np(vert), _np(faces)
    assert np.isnan(vert[V]).all() and (faces[F] == -7).all()
    assert np.isfinite(vert[:V]).all() and (faces[:F] >= 0).all() and (faces[:F] < max(V, 1)).all()
    if cols is not None:
        cols = _np(cols)
        assert np.isnan(cols[V]).all()
        cols = cols[:V]
    return vert[:V], faces[:F], cols, (V, F)


def _colours(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)).astype(np.float32), (rng.random(n) < 0.7).astype(np.float32) * rng.integers(1, 4, n).astype(np.float32)


def _check_extraction(r, grid, tsdf, weight, min_weight, seed, euler=None):
    rgb, cw = _colours(tsdf.size, seed)
    want = tn.extract(grid, tsdf, weight, min_weight, rgb=rgb, cweight=cw)
    v, f, c, (V, F) = _extract(r, grid, tsdf, weight, min_weight, rgb, cw)
    assert (V, F) == (want[0].shape[0], want[1].shape[0])
    assert np.array_equal(f, want[1]) and f.dtype == np.int32
    _same_bits(v, want[0], "vertices")
    _same_bits(c, want[2], "colours")
    inv = tn.mesh_invariants(f, V) if F else None
    if F:
        assert inv["edge_max"] <= 2 and inv["directed_repeats"] == 0 and inv["degenerate_index"] == 0 and inv["unreferenced"] == 0
    if euler is not None:
        assert inv["edge_min"] == 2 and inv["unpaired"] == 0 and inv["euler"] == euler and tn.signed_volume(v, f) > 0
    # without colours: the same geometry
    v2, f2, c2, _ = _extract(r, grid, tsdf, weight, min_weight)
    assert c2 is None and np.array_equal(f2, f)
    _same_bits(v2, v, "vertices without colours")
    return inv


@pytest.mark.parametrize("kind,euler", [("sphere", 2), ("torus", 0), ("zeros", 2), ("half", None), ("offcentre", 2)])
def test_extraction_equals_the_restatement(r, kind, euler):
    grid, tsdf, weight = tn.analytic_grid(kind)
    inv = _check_extraction(r, grid, tsdf, weight, 1.0, seed=3, euler=euler)
    print(kind, inv)
    if kind == "half":
        assert inv["edge_min"] == 1
    if kind == "zeros":
        assert int((tsdf == 0).sum()) == 6
    if kind == "offcentre":
        assert grid["dims"] == (20, 17, 13)


def test_extraction_of_one_cell_and_of_an_integrated_volume(r):
    rng = np.random.default_rng(5)
    one = tn.make_grid((0.25, -0.5, 1.0), 0.5, (2, 2, 2), 1.0)
    for _ in range(6):
        f = rng.uniform(-1, 1, 8).astype(np.float32)
        inv = _check_extraction(r, one, f, np.ones(8, np.float32), 1.0, seed=int(rng.integers(100)))
        assert inv is None or inv["F"] >= 1
    # the integrated scene's volume: real weights (0 .. 3), min_weight 1 and 2
    grid, _, v32, _, _ = _scene()
    for mw in (1.0, 2.0):
        rgbw = tn.extract(grid, v32["tsdf"], v32["weight"], mw, rgb=v32["rgb"], cweight=v32["cweight"])
        v, f, c, _ = _extract(r, grid, v32["tsdf"], v32["weight"], mw, v32["rgb"], v32["cweight"])
        assert np.array_equal(f, rgbw[1]) and f.shape[0] > 0
        _same_bits(v, rgbw[0], "vertices")
        _same_bits(c, rgbw[2], "colours")


def test_all_positive_grid_gives_nothing_and_emit_launches_nothing(r):
    grid, tsdf, weight = tn.analytic_grid("sphere")
    v, f, c, (V, F) = _extract(r, grid, np.abs(tsdf) + np.float32(0.1), weight, 1.0, *_colours(tsdf.size, 1))
    assert (V, F) == (0, 0) and v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)
    # ... and emit after that plan takes no buffer at all
    g = _grid_struct(grid)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    t, w = _dev(np.abs(tsdf) + np.float32(0.1)), _dev(weight)
    nbytes = int(r.lib.gs_tsdf_mesh_workspace_bytes(C.byref(g)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    counts = (C.c_longlong * 2)(-1, -1)
    assert r.lib.gs_tsdf_mesh_plan(r.ctx, C.byref(g), p(t), p(w), C.c_float(1.0), p(ws), nbytes, counts) == 0
    assert list(counts) == [0, 0]
    assert r.lib.gs_tsdf_mesh_emit(r.ctx, C.byref(g), None, None, None, None, C.c_float(1.0), p(ws), None, None, None) == 0
    # what emit refuses: another min_weight or workspace than the plan's; a plan that failed leaves none to emit
    assert r.lib.gs_tsdf_mesh_emit(r.ctx, C.byref(g), p(t), p(w), None, None, C.c_float(2.0), p(ws), None, None, None) == 1
    assert r.lib.gs_tsdf_mesh_emit(r.ctx, C.byref(g), p(t), p(w), None, None, C.c_float(1.0), p(t), None, None, None) == 1
    assert r.lib.gs_tsdf_mesh_plan(r.ctx, C.byref(g), p(t), p(w), C.c_float(1.0), p(ws), nbytes - 256, counts) == 1
    assert r.lib.gs_tsdf_mesh_emit(r.ctx, C.byref(g), p(t), p(w), None, None, C.c_float(1.0), p(ws), None, None, None) == 5
    r.sync()


@pytest.mark.parametrize("dims", [(65, 65, 65), (16, 16, 8)])
def test_scan_carries(r, dims):
    n = dims[0] * dims[1] * dims[2]
    if dims == (65, 65, 65):
        assert -(-n // TSDF_SCAN_TILE) > TSDF_THREADS          # more tiles than one pass of the top-level scan
    else:
        assert n % TSDF_SCAN_TILE == 0 and n // TSDF_SCAN_TILE == 2
    grid = tn.make_grid((-1.0, -1.0, -1.0), 2.0 / (dims[0] - 1), dims, 6.0 / (dims[0] - 1))
    p = tn.lattice_points(grid, np.float64)
    hi = p.max(0)
    centre = 0.5 * (hi - 1.0) + np.array([0.03, -0.02, 0.01])
    d = np.linalg.norm((p - centre) / (0.5 * (hi + 1.0)), axis=1) - 0.8          # an ellipsoid that fills the grid: every tile counts
    tsdf = np.clip(d, -0.2, 0.2).astype(np.float32)
    weight = np.ones(n, np.float32)
    weight[(p[:, 0] > 0.4) & (p[:, 1] > 0.3)] = 0.0
    inv = _check_extraction(r, grid, tsdf, weight, 1.0, seed=9)
    assert inv["F"] > (10000 if n > 100000 else 100)


def _shell_scene():
    """~2000 opaque Gaussians on a sphere shell of radius 0.5 and 8 pinhole cameras of 128 x 128 around it."""
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    N = 2000
    i = np.arange(N) + 0.5
    phi, z = np.pi * (1 + 5 ** 0.5) * i, 1 - 2 * i / N
    rad = np.sqrt(1 - z * z)
    xyz = 0.5 * np.stack([rad * np.cos(phi), rad * np.sin(phi), z], 1)
    rng = np.random.default_rng(11)
    params = dict(xyz=xyz, scales=np.full((N, 3), np.log(0.035)), rotation=np.tile([1.0, 0, 0, 0], (N, 1)),
                  opacity=np.full(N, 5.0), features_dc=rng.uniform(-1.5, 1.5, (N, 1, 3)), features_rest=np.zeros((N, 24, 3)))
    params = {k: torch.as_tensor(v.astype(np.float32), device="cuda") for k, v in params.items()}
    cams = []
    for k in range(8):
        a = 2 * np.pi * k / 8 + 0.2
        eye = (2.2 * np.cos(a), 2.2 * np.sin(a), (-0.9, 0.3, 1.1)[k % 3])
        cams.append(Camera(128, 128, 150.0 + k, 148.0 - k, look_at_c2w(eye), cx=64.0 + 2.5 * (k % 3), cy=62.0 + 1.5 * (k % 2)))
    return params, cams


def test_end_to_end_extract_mesh(r):
    from gaussiansplattingmlx_amd import mesh as M
    params, cams = _shell_scene()
    r.setCameraModel("pinhole")
    got = M.extract_mesh(r, params, cams, resolution=48)
    again = M.extract_mesh(r, params, cams, resolution=48)
    a, b = got.cpu(), again.cpu()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    V, F = a.vertices.shape[0], a.faces.shape[0]
    print("end to end: V", V, "F", F)
    assert V > 500 and F > 1000 and a.colors.shape == (V, 3) and got.vertices.is_cuda and got.faces.dtype == torch.int32
    lo, hi = M.default_bounds(params)
    origin, voxel, dims = M.volume_layout((lo, hi), 48)
    assert max(dims) == 48
    top = origin + voxel * (np.array(dims) - 1)
    assert (a.vertices >= origin - 1e-5).all() and (a.vertices <= top + 1e-5).all()
    rr = np.linalg.norm(a.vertices, axis=1)
    print("vertex radius (shell at 0.5): min", rr.min(), "median", np.median(rr), "max", rr.max())
    assert np.isfinite(a.colors).all()
    # the restatement, fed the depth and colour images read back from the GPU
    grid = tn.make_grid(origin, voxel, dims, 4.0 * voxel)
    views = []
    for cam in cams:
        res = r.renderForward(params, cam, wantDepth=True)
        d = r.expectedDepth(res, 0.5)
        col = res.render.clone()
        s = M.camera_view(cam, d, col)
        views.append(dict(Rt=np.array(list(s.Rt), np.float32).reshape(3, 4), fx=np.float32(s.fx), fy=np.float32(s.fy), cx=np.float32(s.cx),
                          cy=np.float32(s.cy), depth=_np(d).reshape(128, 128), color=_np(col).reshape(128, 128, 3)))
    assert all((v["depth"] > 0).any() and (v["depth"] == 0).any() for v in views)
    vol = tn.integrate(grid, views, tn.empty_volume(grid))
    want = tn.extract(grid, vol["tsdf"], vol["weight"], 1.0, rgb=vol["rgb"], cweight=vol["cweight"])
    assert np.array_equal(a.faces, want[1])
    _same_bits(a.vertices, want[0], "vertices")
    _same_bits(a.colors, want[2], "colours")
    inv = tn.mesh_invariants(a.faces, V)
    assert inv["edge_max"] <= 2 and inv["directed_repeats"] == 0 and inv["unreferenced"] == 0 and inv["degenerate_index"] == 0
    # depth_max turns far depth into holes; no colour volume gives no colours; the camera model is put back
    near = M.extract_mesh(r, params, cams[:2], resolution=24, depth_max=1.9, color=False)
    assert near.colors is None and 0 < near.faces.shape[0]
    r.setCameraModel("fisheye")
    M.extract_mesh(r, params, cams[:1], resolution=16)
    assert r.cameraModel == "fisheye"
    r.setCameraModel("pinhole")
