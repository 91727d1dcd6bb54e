"""The densify / prune event's kernels (csrc/densify.hip) against the numpy restatement of tests/densify_numpy.py, which
tests/test_densify_numpy_cpu.py qualifies without a device, at the structural boundaries of the kernels.

Cases (the lists live in tests/densify_numpy.py):
  scan + plan (dn_tile_sums / dn_tile_offsets / dn_offsets / dn_plan_kernel through densifyOffsets and densifyPlan / densifyPlanRead):
    N = 1, 3, 4, 5, 255 .. 257, 1023 .. 1025, 65 535 .. 65 537, 262 143 .. 262 145 (a scan tile is 1024 counts and the one-workgroup
    kernel takes the tile sums 256 at a time: its carry loop runs a second time from 262 145 on), 524 288, 524 289, 786 433; on
    every mix: random 70 / 10 / 10 / 10, all keep, all prune (total 0), all split and all clone (2048 per tile, a whole wave of one
    class in the byte-packed histogram), one non-keep row first or last (split and prune each), tiles alternating all-prune /
    all-split, the first 256-tile chunk all-prune.  One context takes 786 433, then 1025, then 262 145 (the scratch regrown, then
    reused with its count and histogram words at other offsets), with both maps and a gather at K = 1 and 4 at the large N.
  maps (build_map_kernel, build_map_planned_kernel): every mix at N = 1025 and 262 145, every slot; the plain map for the total
    and three below it, the planned one for capacities of the new count, one above, 2N + 7 and three below -- N - 1, N and 2N + 7
    where nothing applies (the identity) --, slots behind the capacity pre-filled with a sentinel.
  gathers (gather_small_kernel, gather_rows4_kernel, gather_rows_kernel through densifyGather, densifyGatherPlanned and
    densifyGatherPlannedPacked): K = 1 (no row launch), 4 and 16 (rows of 9 and 45 floats: the scalar kernel), 9 and 25 (24 and
    72: the float4 kernel) x N = 1, 257, 1000 on the random and a prune-only mix; from contiguous tensors, from and into a
    GaussModel arena whose capacity is no multiple of four, and from and into hand-built buffers whose features_rest starts 1, 2
    or 3 floats off the 16-byte grid (K = 9, 25: the scalar kernel as the fallback).  Destinations are filled with random data and
    compared WHOLE -- rows behind the new count, pads, the words between and behind the segments must keep their bits.
  noise (densify_noise_kernel; the planned gather draws the same rows inside gather_small_kernel): 1, 255, 256, 257, 4096 rows
    under the seeds 0, 1, 2^32 - 1, 2^32, 2^64 - 1, 20260313.
  classify / accumulate: an [N, 4] scales tensor (stride 4, junk in column 3), denom 0, -1 and 8, the statistic exactly at and one
    ulp beside threshold x denom, raw scales of 89 and -104, raw opacities of +-inf, allowDensify both ways, default and other
    thresholds; accumGradNorm in place (out is accumIn) at N = 1, 255, 256, 257 with components of 1e-25 and 1e20.

Bars.  Integers (offsets, totals, class counts, plan words, maps, actions) and every copied float: the same bits.  scales: the same
bits (one float32 addition).  xyz: rtol 1e-6, atol 1e-7 against float64, test_densify_kernels_match_the_oracle's bar for the
exp() inside the noise scale; the planned forms must then repeat densifyGather's bits when that is fed densifyNoise.  Noise: 1e-5
absolute against the float64 restatement on bit-exact float32 uniforms, the bar of
test_gpu_mcmc.py::test_generator_matches_the_restatement for the same arithmetic; a row's bits must not depend on the row count.
classify: test_densify_kernels_match_the_oracle's exclusion rule (rows within 4e-7 relative of a scale or opacity threshold, under
1e-3 of the rows; the hand-placed rows are not among them).  accumGradNorm: the oracle's bits.

Measured on an MI355X: noise, worst |kernel - float64| over the six seeds x 4096 rows 4.96e-7 (seed 2^64 - 1; 3.2e-7 .. 4.9e-7 by
the seed), 0.05 of the bar; the float32 numpy walk of the same rows 4.86e-7 (tests/test_densify_numpy_cpu.py; it may use half
the bar).  Everything else is a comparison of bits, or xyz at the existing bar.  The whole file takes under six seconds.  No
case failed on the kernels as they are: densify.hip is unchanged.

Mutants (scratch builds, each changing one value and no address or bound; only the matching group run):
  1. dn_tile_offsets_kernel stores `ex` without the carry (-k scan): test_scan_and_plan_match_the_restatement fails at 262145,
     524288, 524289 and 786433 and passes at the fifteen counts below; test_scan_scratch_is_regrown_and_reused fails.
  2. gather_rows4_kernel reads quad 0 instead of quad k (-k gather): test_gather_from_contiguous_tensors and
     test_gather_from_and_into_a_model_arena fail in all twelve cases each of K = 9 and 25 and pass at K = 1, 4 and 16, as does
     test_gather_at_a_large_count (K = 1, 4); test_gather_with_features_rest_off_the_16_byte_grid passes (the one-float kernel).
  3. densify_noise3's first key increment 0x9E3779B9 -> 0x9E3779B8 (-k noise): test_noise_matches_the_restatement fails under
     all six seeds.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_dnk_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dz = _load("densify_numpy")
SENTINEL = -77
PER = dict(xyz=3, features_dc=3, scales=3, rotation=4, opacity=1)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, device):
    return torch.as_tensor(np.array(a), device=device)          # (a copy: the shared references are read-only)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _new_renderer():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box")
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(3, 64, 64, (16, 16), False)


@pytest.fixture(scope="module")
def r():
    rr = _new_renderer()
    yield rr
    rr.close()


@functools.lru_cache(maxsize=24)
def _ref(N, mix):
    """A case's actions, counts, offsets, totals and plan words from the restatement, computed once and shared (read only)."""
    a = dz.actions_of(mix, N)
    off, st = dz.offsets(a)
    for v in (a, off):
        v.setflags(write=False)
    return dict(actions=a, counts=dz.counts_of(a), off=off, st=st, plan=dz.plan(a, N))


# ------------------------------------------------------------------------------------------------------------ scan + plan
def _scan_checks(r, N, mix):
    ref = _ref(N, mix)
    ta, tc = _dev(ref["actions"], r.device), _dev(ref["counts"], r.device)
    goff, gst = r.densifyOffsets(ta, tc)
    assert gst == ref["st"], (N, mix, gst, ref["st"])
    np.testing.assert_array_equal(_np(goff), ref["off"], err_msg=f"{N} {mix}")
    poff = r.densifyPlan(ta, tc)
    plan = r.densifyPlanRead()
    assert [plan[k] for k in dz.PLAN_WORDS] == ref["plan"], (N, mix, plan, ref["plan"])
    np.testing.assert_array_equal(_np(poff), ref["off"], err_msg=f"planned {N} {mix}")
    return ta, tc


@pytest.mark.parametrize("N", dz.SCAN_NS)
def test_scan_and_plan_match_the_restatement(r, N):
    """Offsets, total, class counts and the eight plan words, bit for bit, on every mix."""
    for mix in dz.MIXES:
        _scan_checks(r, N, mix)


def test_scan_scratch_is_regrown_and_reused():
    """One fresh context: 786 433 rows (769 tiles: the scratch is allocated, the carry loop runs four times), then 1025 (two
    tiles on the larger scratch: the count words and the per-tile histogram sit at other offsets), then 262 145 (257 tiles: one
    tile in the loop's second chunk); at the large N both maps as well.  (The module's shared context meets its counts in
    ascending order: there every larger count frees the scratch and allocates it anew.)"""
    r = _new_renderer()
    try:
        for N in (786433, 1025, 262145, 786433):
            for mix in ("random", "chunk0_prune", "all_split", "alternating_tiles"):
                _scan_checks(r, N, mix)
        _map_checks(r, 786433, "random")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------ maps
def _map_into(r, fn, N, ta, toff, count, slack=67):
    """The library's map entry point on tensors of count + slack slots, the slack pre-filled with a sentinel."""
    from gaussiansplattingmlx_amd.renderer import _p
    g = torch.full((count + slack,), SENTINEL, dtype=torch.int32, device=r.device)
    m = torch.full((count + slack,), SENTINEL, dtype=torch.int32, device=r.device)
    r._check(fn(r.ctx, int(N), _p(ta), _p(toff), int(count), _p(g), _p(m)))
    g, m = _np(g), _np(m)
    assert (g[count:] == SENTINEL).all() and (m[count:] == SENTINEL).all(), (N, count)
    return g[:count], m[:count]


def _map_checks(r, N, mix):
    ref = _ref(N, mix)
    a, off, st, words = ref["actions"], ref["off"], ref["st"], ref["plan"]
    ta, tc, toff = _dev(a, r.device), _dev(ref["counts"], r.device), _dev(off, r.device)
    for total in sorted({st["total"], max(st["total"] - 3, 0)}):
        g, m = _map_into(r, r.lib.gs_build_densify_output_map, N, ta, toff, total)
        wg, wm = dz.output_map(a, off, total)
        np.testing.assert_array_equal(g, wg, err_msg=f"gather {N} {mix} total {total}")
        np.testing.assert_array_equal(m, wm, err_msg=f"mode {N} {mix} total {total}")
    r.densifyPlan(ta, tc)
    plan = r.densifyPlanRead()
    assert [plan[k] for k in dz.PLAN_WORDS] == words
    new = words[0]
    caps = (new, new + 1, 2 * N + 7, new - 3) if words[1] else (N - 1, N, 2 * N + 7)
    for cap in caps:
        if cap <= 0:                                            # (a new count of three or less: there is no capacity three below)
            continue
        g, m = _map_into(r, r.lib.gs_build_densify_output_map_planned, N, ta, toff, cap)
        wg, wm = dz.planned_map(a, off, words, cap)
        np.testing.assert_array_equal(g, wg, err_msg=f"planned gather {N} {mix} cap {cap}")
        np.testing.assert_array_equal(m, wm, err_msg=f"planned mode {N} {mix} cap {cap}")
    # the wrapper's own form: `capacity` zero-filled slots
    pg, pm = r.buildDensifyOutputMapPlanned(ta, toff, 2 * N + 7)
    wg, wm = dz.planned_map(a, off, words, 2 * N + 7)
    assert np.array_equal(_np(pg), wg) and np.array_equal(_np(pm), wm)


@pytest.mark.parametrize("mix", dz.MIXES)
@pytest.mark.parametrize("N", dz.MAP_NS)
def test_maps_match_the_restatement(r, N, mix):
    """Every slot of both maps; a row whose slots do not fit the total (or the capacity the planned map clamps it to) writes
    nothing, a plan that does not apply maps the identity below min(N, capacity), and the slots behind keep the sentinel."""
    _map_checks(r, N, mix)


# ------------------------------------------------------------------------------------------------------------ gathers
@functools.lru_cache(maxsize=None)
def _gcase(K, N, mix):
    """A gather case: the model, its event's maps and plan words from the restatement (shared, read only)."""
    p = dz.gather_params(N, K)
    a = dz.actions_of(mix, N)
    off, st = dz.offsets(a)
    words = dz.plan(a, N)
    cap = 2 * N + 7                                           # (odd: no multiple of four)
    wg, wm = dz.output_map(a, off, st["total"])
    pg, pm = dz.planned_map(a, off, words, cap)
    for v in list(p.values()) + [a, off, wg, wm, pg, pm]:
        v.setflags(write=False)
    return dict(K=K, N=N, p=p, actions=a, counts=dz.counts_of(a), off=off, st=st, plan=words, cap=cap, wg=wg, wm=wm, pg=pg, pm=pm,
                seed=20260313 + 131 * N + K, own_noise=bool(words[1] and (words[4] or words[5])))


def _shapes(K):
    return dict(xyz=(3,), features_dc=(1, 3), features_rest=(K - 1, 3), scales=(3,), rotation=(4,), opacity=())


def _random_dest(r, rows, K, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return {k: torch.randn((rows,) + s, generator=g).to(r.device) for k, s in _shapes(K).items()}


def _plan_on_device(r, c):
    """Runs the case's scan + plan on the context (the planned kernels read the plan from it) and checks the planned map."""
    ta, tc = _dev(c["actions"], r.device), _dev(c["counts"], r.device)
    toff = r.densifyPlan(ta, tc)
    plan = r.densifyPlanRead()
    assert [plan[k] for k in dz.PLAN_WORDS] == c["plan"]
    np.testing.assert_array_equal(_np(toff), c["off"])
    pg, pm = r.buildDensifyOutputMapPlanned(ta, toff, c["cap"])
    assert np.array_equal(_np(pg), c["pg"]) and np.array_equal(_np(pm), c["pm"])
    return pg, pm


def _expected_rows(r, c, tp):
    """The rows [0, new count) the planned forms must write, as device tensors: a pure copy of the source rows (torch indexing:
    no kernel of the library) -- and, where the event splits or clones, xyz and scales from densifyGather fed densifyNoise
    (at K = 1), which test_gather_from_contiguous_tensors holds to the restatement."""
    n_new = c["plan"][0]
    idx = _dev(c["pg"][:n_new].astype(np.int64), r.device)
    want = {k: tp[k][idx].clone() for k in tp}
    if c["own_noise"]:
        assert n_new == c["st"]["total"]
        nz = r.densifyNoise(c["seed"], n_new)
        narrow = dict(tp, features_rest=tp["features_rest"][:, :0, :])         # (K = 1: no row launch -- the expectation runs no row kernel)
        got = r.densifyGather(narrow, _dev(c["wg"], r.device), _dev(c["wm"], r.device), nz)
        for k in ("features_dc", "rotation", "opacity"):
            assert torch.equal(got[k], want[k]), k
        want["xyz"], want["scales"] = got["xyz"], got["scales"]
    return want


def _contiguous_checks(r, c):
    p, K, N, st, cap, seed = c["p"], c["K"], c["N"], c["st"], c["cap"], c["seed"]
    total, n_new = st["total"], c["plan"][0]
    tp = {k: _dev(v, r.device) for k, v in p.items()}
    src_before = {k: v.clone() for k, v in tp.items()}
    pg, pm = _plan_on_device(r, c)
    if total > 0:
        gg, gm = _dev(c["wg"], r.device), _dev(c["wm"], r.device)
        # densifyGather with a noise tensor: against the float64 restatement
        nz = r.densifyNoise(seed, total)
        want = dz.gather(p, c["wg"], c["wm"], _np(nz))
        dst = _random_dest(r, total + 5, K, 1)
        before = {k: v.clone() for k, v in dst.items()}
        r.densifyGather(tp, gg, gm, nz, out=dst)
        for k in dz.PARAMS:
            got = _np(dst[k])
            assert np.array_equal(_bits(got[total:]), _bits(_np(before[k])[total:])), k          # rows at and behind the count
            if k == "xyz":
                np.testing.assert_allclose(got[:total], want[k], rtol=1e-6, atol=1e-7)
                if st["split"] or st["clone"]:
                    assert np.abs(got[:total] - p["xyz"][c["wg"]]).max() > 1e-5
            else:
                np.testing.assert_array_equal(_bits(got[:total]), _bits(want[k].astype(np.float32)), err_msg=k)
        # ... and without one: the source rows, bit for bit
        dst0 = _random_dest(r, total + 5, K, 2)
        before0 = {k: v.clone() for k, v in dst0.items()}
        r.densifyGather(tp, gg, gm, None, out=dst0)
        for k in dz.PARAMS:
            got = _np(dst0[k])
            assert np.array_equal(_bits(got[:total]), _bits(p[k][c["wg"]])), k
            assert np.array_equal(_bits(got[total:]), _bits(_np(before0[k])[total:])), k
    # the planned gather: the same bits in rows [0, new count), the rows behind untouched
    want = _expected_rows(r, c, tp)
    if not c["own_noise"]:                                     # prune-only, or nothing applies: a copy, no noise
        for k in dz.PARAMS:
            assert np.array_equal(_bits(_np(want[k])), _bits(p[k][c["pg"][:n_new]])), k
    dst = _random_dest(r, cap, K, 3)
    expect = {k: v.clone() for k, v in dst.items()}
    for k in expect:
        expect[k][:n_new] = want[k]
    r.densifyGatherPlanned(tp, pg, pm, seed, dst, cap)
    for k in dz.PARAMS:
        assert torch.equal(dst[k].view(torch.int32), expect[k].view(torch.int32)), k
    # ... and into a packed arena: every word of the buffer
    _packed_checks(r, c, tp, pg, pm, want)
    for k in tp:
        assert torch.equal(tp[k].view(torch.int32), src_before[k].view(torch.int32)), k


def _packed_layout(n, K, order):
    per = dict(PER, features_rest=3 * (K - 1))
    starts, off = {}, 0
    for k in order:
        starts[k] = off
        off += (n * per[k] + 3) & ~3
    return starts, per, off


def _packed_checks(r, c, tp, pg, pm, want, base=None):
    from gaussiansplattingmlx_amd.trainer import ARENA_ORDER
    n_new, cap, K = c["plan"][0], c["cap"], c["K"]
    if base is None:
        base = torch.randn(_packed_layout(cap, K, ARENA_ORDER)[2] + 64, generator=torch.Generator().manual_seed(4)).to(r.device)
    else:
        base.copy_(torch.randn(base.numel(), generator=torch.Generator().manual_seed(4)))
    expect = base.clone()
    starts, per, _ = _packed_layout(n_new, K, ARENA_ORDER)
    for k in ARENA_ORDER:
        expect[starts[k]:starts[k] + n_new * per[k]] = want[k].reshape(-1)
    r.densifyGatherPlannedPacked(tp, pg, pm, c["seed"], base, cap, ARENA_ORDER)
    assert torch.equal(base.view(torch.int32), expect.view(torch.int32)), (K, c["N"])


@pytest.mark.parametrize("mix", dz.GATHER_MIXES)
@pytest.mark.parametrize("N", dz.GATHER_NS)
@pytest.mark.parametrize("K", dz.GATHER_KS)
def test_gather_from_contiguous_tensors(r, K, N, mix):
    _contiguous_checks(r, _gcase(K, N, mix))


@pytest.mark.parametrize("K", [1, 4])
def test_gather_at_a_large_count(r, K):
    """786 433 rows in, ~865 000 out: rows behind the scan's second and third chunk, at the widths that need no 700 k-row SH tensor."""
    _contiguous_checks(r, _gcase(K, 786433, "random"))
    _gcase.cache_clear()


@pytest.mark.parametrize("mix", dz.GATHER_MIXES)
@pytest.mark.parametrize("N", dz.GATHER_NS)
@pytest.mark.parametrize("K", dz.GATHER_KS)
def test_gather_from_and_into_a_model_arena(r, K, N, mix):
    """The trainer's forms: sources are the views of a GaussModel arena (capacity 2N + 7), destinations its other buffer -- packed
    for densifyGather, at capacity strides for the planned gather, laid out on the device for the packed planned one.  Pads and
    unused rows hold random data on both sides; both buffers are compared whole."""
    from gaussiansplattingmlx_amd.trainer import ARENA_ORDER, GaussModel
    c = _gcase(K, N, mix)
    cap, n_new, total = c["cap"], c["plan"][0], c["st"]["total"]
    model = GaussModel({k: _dev(v, r.device) for k, v in c["p"].items()}, r.device, capacity=cap)
    src = model._pbuf[model._cur]
    noise = torch.randn(src.numel(), generator=torch.Generator().manual_seed(5)).to(r.device)
    mask = torch.zeros(src.numel(), dtype=torch.bool, device=r.device)
    for k, off in zip(ARENA_ORDER, model.seg_start):
        mask[int(off):int(off) + N * model._per[k]] = True
    src.copy_(torch.where(mask, src, noise))
    src_before = src.clone()
    tp = model.getParams()
    for k in dz.PARAMS:
        assert np.array_equal(_bits(_np(tp[k])), _bits(c["p"][k])), k
    pg, pm = _plan_on_device(r, c)
    want = _expected_rows(r, c, tp)

    def staged(views_of):
        views = views_of()
        other = model._pbuf[1 - model._cur]
        other.copy_(torch.randn(other.numel(), generator=torch.Generator().manual_seed(6)))
        model._staged = None
        return views, other, other.clone()

    if total > 0 and c["own_noise"]:                            # densifyGather into the packed layout of `total` rows
        views, other, expect = staged(lambda: model.stagingViews(total))
        for k, off in zip(ARENA_ORDER, model._offsets(total)[0]):
            expect[off:off + total * model._per[k]] = want[k].reshape(-1)
        r.densifyGather(tp, _dev(c["wg"], r.device), _dev(c["wm"], r.device), r.densifyNoise(c["seed"], total), out=views)
        assert torch.equal(other.view(torch.int32), expect.view(torch.int32))
    views, other, expect = staged(lambda: model.stagingViews(cap, stride=cap))          # the planned gather: capacity strides
    for k, off in zip(ARENA_ORDER, model._offsets(cap)[0]):
        expect[off:off + n_new * model._per[k]] = want[k].reshape(-1)
    r.densifyGatherPlanned(tp, pg, pm, c["seed"], views, cap)
    assert torch.equal(other.view(torch.int32), expect.view(torch.int32))
    base = model.stagingBase(cap)                                                       # the packed planned gather
    model._staged = None
    assert base.numel() >= _packed_layout(cap, K, ARENA_ORDER)[2]
    _packed_checks(r, c, tp, pg, pm, want, base=base)
    assert torch.equal(src.view(torch.int32), src_before.view(torch.int32))


def _flat_views(buf, rows, K, frest_off):
    """The six tensors as views of one flat buffer, two unused words between them, features_rest starting frest_off floats
    behind a 16-byte boundary.  Returns (views, {name: (start, floats)})."""
    per = dict(PER, features_rest=3 * (K - 1))
    views, where, off = {}, {}, 1
    for k in ("xyz", "scales", "rotation", "opacity", "features_dc", "features_rest"):
        off += 2
        if k == "features_rest":
            off = ((off + 3) & ~3) + frest_off
        n = rows * per[k]
        assert off + n <= buf.numel()
        views[k] = buf[off:off + n].view((rows,) + _shapes(K)[k])
        where[k] = (off, n)
        off += n
    assert (views["features_rest"].data_ptr() - buf.data_ptr()) // 4 % 4 == frest_off and buf.data_ptr() % 16 == 0
    return views, where


@pytest.mark.parametrize("offs", [(1, 1), (2, 2), (3, 3), (0, 1), (2, 0)], ids=lambda o: f"src{o[0]}_dst{o[1]}")
@pytest.mark.parametrize("N", dz.GATHER_NS)
@pytest.mark.parametrize("K", [9, 25])
def test_gather_with_features_rest_off_the_16_byte_grid(r, K, N, offs):
    """Rows of a multiple of four floats between tensors that are NOT both 16-byte aligned: launch_gather_rows must fall back to
    the one-float kernel.  Source and destination are views of hand-built flat buffers full of random data, compared whole."""
    from gaussiansplattingmlx_amd.renderer import GsplatError
    from gaussiansplattingmlx_amd.trainer import ARENA_ORDER
    so, do = offs
    c = _gcase(K, N, "random")
    cap, n_new, total = c["cap"], c["plan"][0], c["st"]["total"]
    floats = lambda rows: rows * (14 + 3 * (K - 1)) + 64
    src = torch.randn(floats(N), generator=torch.Generator().manual_seed(7)).to(r.device)
    tp, _ = _flat_views(src, N, K, so)
    for k in dz.PARAMS:
        tp[k].copy_(_dev(c["p"][k], r.device))
    src_before = src.clone()
    pg, pm = _plan_on_device(r, c)
    want = _expected_rows(r, c, {k: _dev(v, r.device) for k, v in c["p"].items()})
    if total > 0:                                               # densifyGather with the library's noise
        dst = torch.randn(floats(total), generator=torch.Generator().manual_seed(8)).to(r.device)
        views, where = _flat_views(dst, total, K, do)
        expect = dst.clone()
        if c["own_noise"]:
            for k, (off, n) in where.items():
                expect[off:off + n] = want[k].reshape(-1)
            r.densifyGather(tp, _dev(c["wg"], r.device), _dev(c["wm"], r.device), r.densifyNoise(c["seed"], total), out=views)
            assert torch.equal(dst.view(torch.int32), expect.view(torch.int32))
    dst = torch.randn(floats(cap), generator=torch.Generator().manual_seed(9)).to(r.device)          # the planned gather
    views, where = _flat_views(dst, cap, K, do)
    expect = dst.clone()
    for k, (off, n) in where.items():
        expect[off:off + n_new * (n // cap)] = want[k].reshape(-1)
    r.densifyGatherPlanned(tp, pg, pm, c["seed"], views, cap)
    assert torch.equal(dst.view(torch.int32), expect.view(torch.int32))
    if so:                                                      # packed: the base is aligned by contract, the source is not
        _packed_checks(r, c, tp, pg, pm, want)
        base = torch.zeros(_packed_layout(cap, K, ARENA_ORDER)[2] + 8, device=r.device)
        with pytest.raises(GsplatError):                        # (a base off the grid is refused, not gathered into)
            r.densifyGatherPlannedPacked(tp, pg, pm, c["seed"], base[1:], cap, ARENA_ORDER)
        assert not bool(base.any())
    assert torch.equal(src.view(torch.int32), src_before.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ noise
@pytest.mark.parametrize("seed", dz.NOISE_SEEDS)
def test_noise_matches_the_restatement(r, seed):
    """densify_noise3 is Philox4x32-10 of (row, 0, 'dens', 'ify!') under the seed's two halves, Box-Muller on float32 uniforms:
    within 1e-5 of the float64 restatement (a wrong round constant, key bump or counter word gives other numbers altogether),
    and row j has the same bits whatever the row count is."""
    rows = max(dz.NOISE_ROWS)
    full = _np(r.densifyNoise(seed, rows))
    want = dz.densify_noise(seed, rows)
    worst = float(np.abs(full.astype(np.float64) - want).max())
    print(f"densify noise seed {seed}: worst |kernel - float64| {worst:.3e}")
    assert np.isfinite(full).all() and worst <= dz.NOISE_BAR, worst
    for n in dz.NOISE_ROWS:
        z = _np(r.densifyNoise(seed, n))
        assert z.shape == (n, 3) and np.array_equal(_bits(z), _bits(full[:n])), n


# ------------------------------------------------------------------------------------------------------------ classify / accumulate
@pytest.mark.parametrize("th", dz.CLASSIFY_THRESHOLDS, ids=["default", "other"])
def test_classify_at_stride_four_and_at_its_edges(r, oracle32, th):
    acc, scales, opacity = dz.classify_inputs(th)
    assert scales.shape[1] == 4
    near = dz.classify_near(th, scales, opacity)
    assert near.mean() < 1e-3 and not near[:48].any()
    ta, ts, to = _dev(acc, r.device), _dev(scales, r.device), _dev(opacity, r.device)
    seen = set()
    for denom in dz.CLASSIFY_DENOMS:
        for allow in (True, False):
            wa, wc = oracle32.classify_gaussians(acc, denom, scales, opacity, allowDensify=allow, **th)
            ga, gc = r.classifyGaussians(ta, denom, ts, to, allowDensify=allow, **th)
            np.testing.assert_array_equal(_np(ga)[~near], wa[~near], err_msg=f"denom {denom} allow {allow}")
            np.testing.assert_array_equal(_np(gc)[~near], wc[~near], err_msg=f"denom {denom} allow {allow}")
            np.testing.assert_array_equal(_np(gc), dz.counts_of(_np(ga)))
            seen |= set(np.unique(wa).tolist()) if denom > 0 and allow else set()
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("N", dz.ACCUM_NS)
def test_accumulate_in_place(r, oracle32, N):
    """accum_grad_norm_kernel with accumOut == accumIn (how the trainer runs it through gs_set_grad_norm_accum), twice, with
    components whose squares underflow and overflow: the oracle's bits."""
    g, acc = dz.accum_inputs(N)
    tg, t = _dev(g, r.device), _dev(acc, r.device).clone()
    want = acc
    for _ in range(2):
        out = r.accumGradNorm(tg, t, out=t)
        assert out is t
        want = oracle32.accum_grad_norm(g, want)
        np.testing.assert_array_equal(_bits(_np(t)), _bits(want))
    assert torch.equal(tg, _dev(g, r.device))
