"""Mesh extraction without a GPU: the numpy restatement of TSDF fusion and marching tetrahedra
(tests/tsdf_numpy.py) on analytic volumes, its float32 form against its float64 form, the mesh PLY and the host-side refusals.

What a closed surface must satisfy, checked on index arrays alone: every undirected edge lies in exactly two triangles, every
directed edge appears once and its reverse once (a consistent winding), no triangle repeats an index, no vertex is unreferenced,
and V - E + F is the surface's Euler characteristic.  The winding rule is combinatorial, so all of it holds on the grid that
puts six lattice points exactly on the surface (zero-area triangles), where a winding taken from positions would not.

Recorded (the restatement, float32 and float64 alike): sphere V = 614, F = 1224; torus V = 724, F = 1448; exact zeros V = 182,
F = 360; half observed V = 286, F = 528 with 42 boundary edges.  Integrate scene (20 x 17 x 13, three 96 x 80 views): float32
and float64 take the same pixel and truncation decisions on every voxel (share that differ 0; the cap is 0.5 %), and where they
agree tsdf differs by at most 6.7e-7, colour by 6e-8, the weights not at all (bar 1e-5)."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_tsdfc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


tn = _load("tsdf_numpy")

CLOSED = {"sphere": (2, 614, 1224), "torus": (0, 724, 1448), "zeros": (2, None, None)}


def _assert_closed(inv, euler):
    assert inv["edge_min"] == 2 and inv["edge_max"] == 2, inv
    assert inv["directed_repeats"] == 0 and inv["unpaired"] == 0, inv
    assert inv["degenerate_index"] == 0 and inv["unreferenced"] == 0, inv
    assert inv["euler"] == euler, inv


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", sorted(CLOSED))
def test_closed_surfaces_are_manifold_and_consistently_wound(kind, dtype):
    grid, tsdf, weight = tn.analytic_grid(kind)
    v, f, _ = tn.extract(grid, tsdf, weight, 1.0, dtype=dtype)
    inv = tn.mesh_invariants(f, len(v))
    print(kind, dtype.__name__, inv)
    euler, V, F = CLOSED[kind]
    _assert_closed(inv, euler)
    if V is not None:
        assert (inv["V"], inv["F"]) == (V, F)
    assert v.dtype == dtype and f.dtype == np.int32 and np.isfinite(v).all()
    assert tn.signed_volume(v, f) > 0            # counter-clockwise seen from outside: the enclosed volume is positive
    lo = grid["origin"].astype(np.float64)
    hi = lo + float(grid["voxel"]) * (np.array(grid["dims"]) - 1)
    assert (v >= lo - 1e-6).all() and (v <= hi + 1e-6).all()


def test_exact_zeros_give_zero_area_triangles_with_the_neighbours_winding():
    grid, tsdf, weight = tn.analytic_grid("zeros")
    assert int((tsdf == 0).sum()) == 6           # (+-0.5, 0, 0) and its permutations lie on the radius-0.5 sphere exactly
    v, f, _ = tn.extract(grid, tsdf, weight, 1.0, dtype=np.float64)
    tri = v[f]
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert int((area == 0).sum()) > 0            # the case is what it claims to be
    _assert_closed(tn.mesh_invariants(f, len(v)), 2)


def test_half_observed_volume_gives_an_open_manifold():
    grid, tsdf, weight = tn.analytic_grid("half")
    v, f, _ = tn.extract(grid, tsdf, weight, 1.0)
    inv = tn.mesh_invariants(f, len(v))
    print("half", inv)
    assert inv["F"] > 0 and inv["edge_max"] == 2 and inv["edge_min"] == 1       # boundary edges exist, none is shared by three
    assert inv["directed_repeats"] == 0 and inv["degenerate_index"] == 0 and inv["unreferenced"] == 0
    assert (v[:, 0] >= 0.05 - 1e-6).all()                                      # nothing from the unobserved half
    full = tn.extract(grid, tsdf, np.ones_like(weight), 1.0)[1]
    assert inv["F"] < full.shape[0]


def test_nothing_observed_or_nothing_inside_gives_an_empty_mesh():
    grid, tsdf, weight = tn.analytic_grid("sphere")
    for f_, w_ in ((tsdf, np.zeros_like(weight)), (np.abs(tsdf) + 0.1, weight)):
        v, f, c = tn.extract(grid, f_, w_, 1.0, rgb=np.zeros((tsdf.size, 3), np.float32), cweight=np.zeros_like(weight))
        assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)


def test_case_table_lists_reversed_triangles_for_the_complemented_case():
    """An odd tetrahedron takes the complemented case: it must list the same triangles, reversed, with the same diagonal."""
    for m in range(1, 15):
        a, b = tn.TRI[m], tn.TRI[15 - m]
        assert tn.NTRI[m] == tn.NTRI[15 - m] == (2 if bin(m).count("1") == 2 else 1)
        if tn.NTRI[m] == 1:
            assert list(b[0]) == list(a[0][::-1])
        else:       # (c0, c1, c2), (c0, c2, c3) against (c0, c3, c2), (c0, c2, c1): the other way round, the same diagonal
            assert list(b[0]) == [a[1][0], a[1][2], a[1][1]] and list(b[1]) == [a[0][0], a[0][2], a[0][1]]


def test_vertex_colours_interpolate_and_fall_back():
    grid, tsdf, weight = tn.analytic_grid("sphere")
    n = tsdf.size
    rng = np.random.default_rng(1)
    rgb = rng.random((n, 3)).astype(np.float32)
    cw = (rng.random(n) < 0.6).astype(np.float32)
    v, f, c = tn.extract(grid, tsdf, weight, 1.0, rgb=rgb, cweight=cw)
    assert c.shape == v.shape and np.isfinite(c).all() and (c >= 0).all() and (c <= 1).all()
    assert int((c == 0.5).all(1).sum()) > 0                            # both endpoints without a colour
    c1 = tn.extract(grid, tsdf, weight, 1.0, rgb=rgb, cweight=np.ones(n, np.float32))[2]
    assert not (c1 == 0.5).all(1).any()


def test_float32_integration_against_float64():
    grid, views = tn.integrate_scene(3)
    d32, d64 = [], []
    v32 = tn.integrate(grid, views, tn.empty_volume(grid), np.float32, d32)
    v64 = tn.integrate(grid, views, tn.empty_volume(grid, dtype=np.float64), np.float64, d64)
    agree = np.ones(v32["tsdf"].shape, bool)
    for a, b in zip(d32, d64):
        for x, y in zip(a, b):
            agree &= x == y
    share = 1.0 - float(agree.mean())
    print("share of voxels whose pixel or truncation decisions differ", share)
    assert share <= 0.005
    for k in ("tsdf", "weight", "rgb", "cweight"):
        err = float(np.abs(v32[k][agree].astype(np.float64) - v64[k][agree]).max())
        print(k, err)
        assert err <= 1e-5
    # the scene exercises what it is for: observed and unobserved voxels, fronts and interiors, holes, more than one view
    w = v32["weight"]
    assert (w == 0).any() and (w >= 2).any() and (v32["tsdf"] < 0).any() and (v32["tsdf"] == 1).any()
    assert (v32["cweight"] < w).any() and np.isfinite(v32["tsdf"]).all() and np.isfinite(v32["rgb"]).all()
    assert v32["tsdf"].dtype == np.float32


def test_views_in_batches_equal_views_one_by_one_in_the_restatement():
    grid, views = tn.integrate_scene(5)
    a = tn.integrate(grid, views, tn.empty_volume(grid))
    b = tn.empty_volume(grid)
    for vw in views:
        tn.integrate(grid, [vw], b)
    for k in a:
        assert np.array_equal(a[k], b[k])


def test_mesh_ply_round_trip(tmp_path):
    from gaussiansplattingmlx_amd.ply import read_mesh_ply, write_mesh_ply
    grid, tsdf, weight = tn.analytic_grid("torus")
    rgb = np.random.default_rng(0).random((tsdf.size, 3)).astype(np.float32)
    v, f, c = tn.extract(grid, tsdf, weight, 1.0, rgb=rgb, cweight=np.ones_like(weight))
    path = tmp_path / "mesh.ply"
    write_mesh_ply(path, v, f, c)
    head = path.read_bytes().split(b"end_header\n")[0].decode().split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    assert "property list uchar int vertex_indices" in head and "property uchar red" in head
    assert path.stat().st_size == len("\n".join(head)) + len("end_header\n") + 15 * len(v) + 13 * len(f)
    v2, f2, c2 = read_mesh_ply(path)
    assert np.array_equal(v2, v) and np.array_equal(f2, f) and v2.dtype == np.float32 and f2.dtype == np.int32
    assert np.array_equal(c2, np.floor(np.clip(c.astype(np.float64), 0, 1) * 255 + 0.5).astype(np.uint8))
    write_mesh_ply(path, v, f)                                          # no colours: mid grey
    assert (read_mesh_ply(path)[2] == 128).all()
    write_mesh_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert [x.shape for x in read_mesh_ply(path)] == [(0, 3)] * 3
    with pytest.raises(ValueError):
        write_mesh_ply(path, v, f + len(v))
    write_mesh_ply(path, v, f, c)
    path.write_bytes(path.read_bytes()[:-3])
    with pytest.raises(ValueError):
        read_mesh_ply(path)


def test_refusals_need_no_gpu():
    from gaussiansplattingmlx_amd.camera import Camera, look_at_c2w
    from gaussiansplattingmlx_amd.mesh import TSDFVolume, extract_mesh, volume_layout
    fisheye = Camera(64, 64, 50.0, 50.0, look_at_c2w((2.0, 0.0, 0.5)), model="fisheye")
    with pytest.raises(ValueError, match="fisheye"):
        extract_mesh(None, {}, [fisheye])
    for dims in ((1, 8, 8), (8, 1025, 8), (8, 8), (1024, 1024, 512)):
        with pytest.raises(ValueError):
            TSDFVolume(None, (0, 0, 0), 0.1, dims, 0.3)
    with pytest.raises(ValueError):
        TSDFVolume(None, (0, 0, 0), 0.0, (8, 8, 8), 0.3)
    origin, voxel, dims = volume_layout(((-1, -0.5, 0), (1, 0.5, 0.25)), 41)
    assert dims == (41, 21, 6) and abs(voxel - 0.05) < 1e-12 and tuple(origin) == (-1, -0.5, 0)
    assert all(origin[a] + voxel * (dims[a] - 1) >= hi - 1e-9 for a, hi in enumerate((1, 0.5, 0.25)))


def test_abi_entry_points_check_their_arguments_without_a_gpu():
    import ctypes as C
    from gaussiansplattingmlx_amd import _lib, build
    build.build()
    lib = _lib.load()
    g = _lib.gs_tsdf_grid()
    g.voxel, g.trunc, g.nx, g.ny, g.nz = 0.1, 0.3, 20, 17, 13
    n = 20 * 17 * 13
    tiles = -(-n // 1024)
    al = lambda b: (b + 255) & ~255      # noqa: E731
    assert lib.gs_tsdf_mesh_workspace_bytes(C.byref(g)) == al(7 * n) + al(n) + 2 * al(4 * n) + 2 * al(8 * tiles) + 256
    g.nx = 1
    assert lib.gs_tsdf_mesh_workspace_bytes(C.byref(g)) == 0
    g.nx, g.ny, g.nz = 1024, 1024, 512
    assert lib.gs_tsdf_mesh_workspace_bytes(C.byref(g)) == 0
    assert lib.gs_tsdf_integrate(None, C.byref(g), 1, None, None, None, None, None) == 1
    assert lib.gs_tsdf_mesh_plan(None, C.byref(g), None, None, 1.0, None, 0, None) == 1
    assert lib.gs_tsdf_mesh_emit(None, C.byref(g), None, None, None, None, 1.0, None, None, None, None) == 1
    assert C.sizeof(_lib.gs_tsdf_grid) == 32 and C.sizeof(_lib.gs_tsdf_view) == 88
