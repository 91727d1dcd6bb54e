"""The MCMC event on the device (csrc/mcmc.hip mcmc_block_sums_kernel, mcmc_block_offsets_kernel, mcmc_compact_kernel,
mcmc_sample_kernel, mcmc_formula_kernel, mcmc_copy_kernel) against mcmc_numpy.event, the float64 restatement of a whole event, at
the sizes, row widths, layouts and draw counts where the scan carry, the compaction, the n_max clamp, the row decode and the
scratch reuse can go wrong.

Every case compares the WHOLE state after the event -- the parameter buffer and both moment buffers, pad rows, segment pads
and spare words included -- with the restatement.  Bars, fixed before the first run:

  * every draw's source is the restatement's.  No draw is excused: each case asserts on the host, before the device runs, that
    no draw's target lies within GAP = 1e-9 of the total from a prefix entry (mcmc_numpy.min_boundary_gap).  The device's
    prefix differs from numpy's cumsum by the summation order alone, about N 2^-53 = 8e-12 of the total at N = 70 001; a seed
    that misses the condition is passed over for the next one (_seed_with_gap);
  * the opacity and the scales of a source: within 1 float32 ulp of the restatement's float64 value rounded to float32 (the
    formula is held to 1e-9 in test_mcmc_cpu.py; the kernel works in float64 and rounds once, so 1 ulp allows a rounding tie);
  * a destination: its source's row on the device, bit for bit;
  * every other float of the three buffers: the restatement's, bit for bit (moments zero on the touched rows, everything else
    the input's, NaN payloads included);
  * a second run from the same state: the same bits.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
GAP = 1e-9
TILE = 1024                      # csrc/mcmc.hip MC_TILE: rows per block of the scan kernels, four consecutive rows per thread
NAN_A, NAN_B = 0x7FC12345, 0xFFC00001       # two NaNs with a payload


def _load(name):
    spec = importlib.util.spec_from_file_location("_mcmce_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mn = _load("mcmc_numpy")
KEYS = mn.KEYS


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X box")


@pytest.fixture(scope="module")
def renderer():
    """One context for the whole file: its event scratch is grown, kept and reused from case to case."""
    _gpu()
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    return GaussianRenderer(4, 160, 120, (16, 16), False)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ulps(a, b):
    """The distance of two finite float32 arrays in units in the last place."""
    def key(x):
        i = _bits(x).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ------------------------------------------------------------------------------------------------------------- scenes
def _rows(seed, N, K=16):
    """N rows whose position, colour and rotation floats are all distinct (float i F + e, e the float's place in its row of
    F = 14 + 3 (K - 1)): a copy from another row, or of another element of the right row, shows.  Every opacity is live."""
    rng = np.random.default_rng(seed)
    shapes = dict(xyz=(3,), features_dc=(1, 3), features_rest=(K - 1, 3), scales=(3,), rotation=(4,), opacity=())
    F = 14 + 3 * (K - 1)
    p, e0 = {}, 0
    for k in KEYS:
        per = int(np.prod(shapes[k])) if shapes[k] else 1
        p[k] = (np.arange(N, dtype=np.int64)[:, None] * F + e0 + np.arange(per)[None, :]).reshape((N,) + shapes[k])
        e0 += per
    assert e0 == F and N * F < 2 ** 24                    # (every such integer is a float32)
    p = {k: np.ascontiguousarray(x, np.float32) for k, x in p.items()}
    p["scales"] = rng.normal(-3, 0.7, (N, 3)).astype(np.float32)
    p["opacity"] = rng.uniform(-4, 3, N).astype(np.float32)
    return p


def _placed(N):
    """The rows every sized scene kills on purpose: 3 and 4 (a thread's last row and the next thread's first), 1023 and 1024
    (a block's last row and the next block's first), the last row, one whole thread (rows 8 .. 11) and one whole block (rows
    1024 .. 2047), each where N has room for it and leaves a live row."""
    rows = {3, 4, TILE - 1, TILE, N - 1}
    if N >= TILE - 1:
        rows |= set(range(8, 12))
    if N >= 2 * TILE:
        rows |= set(range(TILE, 2 * TILE))
    return np.array(sorted(r for r in rows if 0 <= r < N), np.int64)


def _scene(seed, N, K=16, extra_dead=0):
    """_rows with the placed rows and `extra_dead` random ones dead (raw -14 .. -6: o below min_opacity = 0.005, raw -5.29),
    and a few dominant weights among the live ones."""
    p = _rows(seed, N, K)
    rng = np.random.default_rng(seed + 1)
    dead = _placed(N)
    if extra_dead:
        dead = np.union1d(dead, rng.choice(N, extra_dead, replace=False))
    p["opacity"][dead] = rng.uniform(-14, -6, dead.size).astype(np.float32)
    live = np.setdiff1d(np.arange(N), dead)
    p["opacity"][live[::97][:5]] = 6.0
    return p, dead


# ------------------------------------------------------------------------------------------------------------- arenas
def _arena(p, stride=None, seed=5):
    """A GaussModel of p's rows at `stride` rows per tensor (default: packed), every other float of its three buffers --
    moments, the rows between N and the stride, the pads behind the segments, the spare words -- a random value."""
    from gaussiansplattingmlx_amd.trainer import GaussModel
    m = GaussModel(p, torch.device("cuda"))
    m.restride(stride or m.N)
    rng = np.random.default_rng(seed)
    rows = {k: x.clone() for k, x in m.getParams().items()}
    for buf, draw in ((m._pbuf[m._cur], rng.normal), (m._mbuf, rng.normal), (m._vbuf, rng.uniform)):
        buf.copy_(torch.as_tensor(draw(0, 1, buf.numel()).astype(np.float32)))
    for k in KEYS:
        m.getParams()[k].copy_(rows[k])
    return m


def _flat(model):
    """The three buffers whole: [parameters, m, v] as numpy."""
    return [b.detach().cpu().numpy().copy() for b in (model._pbuf[model._cur], model._mbuf, model._vbuf)]


def _carve(model, flat, n):
    """Views of n rows of the six tensors into a flat numpy buffer of the model's layout."""
    from gaussiansplattingmlx_amd.trainer import ARENA_ORDER
    starts, _ = model._offsets(model.stride)
    return {k: flat[off:off + n * model._per[k]].reshape((n,) + model._row[k]) for k, off in zip(ARENA_ORDER, starts)}


def _rows_of(model, flat):
    N = model.N
    return tuple({k: x.copy() for k, x in _carve(model, f, N).items()} for f in flat)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{what}: {bad.size} floats differ, the first at {bad[:8].tolist()}: {got[bad[:4]]} for {want[bad[:4]]}"


# ------------------------------------------------------------------------------------------------------------- one event
def _draws(p, mode, cfg, n_add):
    from gaussiansplattingmlx_amd.mcmc import grown_count
    N = p["opacity"].size
    o = mn.sigmoid(p["opacity"])
    cand = np.isfinite(p["opacity"]) & ((o > cfg.min_opacity) if mode == 0 else (o > 0))
    if mode == 0:
        return int((~cand).sum()), int(cand.sum())
    return (grown_count(N, cfg.cap_max, cfg.grow_rate) - N if n_add is None else n_add), int(cand.sum())


def _seed_with_gap(p, mode, cfg, t, first, n_add=None):
    """The first seed from `first` on whose draws all keep GAP from every prefix entry (the module docstring)."""
    n_draw, n_cand = _draws(p, mode, cfg, n_add)
    if n_draw <= 0 or n_cand == 0:
        return first
    for seed in range(first, first + 64):
        _, target, cdf, _, _ = mn.draw(p["opacity"], mode, cfg.min_opacity, n_draw, seed, t)
        if mn.min_boundary_gap(cdf, target) >= GAP:
            return seed
    pytest.fail("no seed in 64 keeps the gap")


def _call(r, model, mode, prm):
    if mode == 0:
        return r.mcmcRelocate(model.getParams(), model.arena, model.m, model.v, prm)
    return r.mcmcGrow(model.getParams(), model.stride, model.arena, model.m, model.v, prm)


def _compare(model, before, got, e):
    """The three buffers after the event against the restatement e of the event on `before` (the module docstring's bars)."""
    n1 = e["N"]
    want = [b.copy() for b in before]
    for flat, rows in zip(want, (e["p"], e["m"], e["v"])):
        views = _carve(model, flat, n1)
        for k in KEYS:
            views[k][...] = rows[k]
    _same_bits(got[1], want[1], "m")
    _same_bits(got[2], want[2], "v")
    gv, wv = _carve(model, got[0], n1), _carve(model, want[0], n1)
    src, dst, s_rows = e["sources"], e["dests"], np.nonzero(e["counts"])[0]
    for k in ("opacity", "scales"):
        assert np.isfinite(gv[k][s_rows]).all(), k
        d = _ulps(gv[k][s_rows], wv[k][s_rows])
        assert d.size == 0 or d.max() <= 1, (k, int(d.max()), s_rows[np.nonzero(d.reshape(s_rows.size, -1).max(1) > 1)[0][:8]])
    for k in KEYS:
        assert np.array_equal(_bits(gv[k][dst]), _bits(gv[k][src])), k           # a destination: its source's row on the device
    for k in ("opacity", "scales"):                        # (what the two bars above have held leaves the whole-buffer comparison)
        wv[k][s_rows] = gv[k][s_rows]
        wv[k][dst] = gv[k][dst]
    _same_bits(got[0], want[0], "parameters")              # every draw's source is the restatement's: the rows are distinct


def _run(r, p, mode, cfg, t, first_seed, stride=None, n_add=None, repeat=True, placed=None, host_check=None):
    """One event of `mode` on an arena of p's rows, compared whole with the restatement; returns (restatement, device result,
    the device's rows after the event).  The preconditions are asserted on the host before the device runs: the placed rows
    are dead, the draws keep the gap, and what host_check(restatement) asks."""
    seed = _seed_with_gap(p, mode, cfg, t, first_seed, n_add)
    model = _arena(p, stride)
    before = _flat(model)
    e = mn.event(*_rows_of(model, before), mode, cfg, t, seed, n_add)
    if placed is not None and mode == 0:
        assert np.isin(placed, e["dests"]).all() or e["stats"]["live"] == 0
    assert mn.min_boundary_gap(e["cdf"], e["target"]) >= GAP
    if host_check is not None:
        host_check(e)
    prm = cfg.params(t, seed)
    res = _call(r, model, mode, prm)
    got = _flat(model)
    if mode == 0:
        assert res == e["stats"], (res, e["stats"])
    else:
        assert res == e["N"], (res, e["N"])
    _compare(model, before, got, e)
    if repeat:
        again = _arena(p, stride)
        assert _call(r, again, mode, prm) == res
        for a, b, what in zip(_flat(again), got, ("parameters", "m", "v")):
            _same_bits(a, b, "second run, " + what)
    return e, res, _carve(model, got[0], e["N"])


def _cfg(N, rate=0.05):
    """The defaults with a cap_max above any grown count."""
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    return MCMCConfig(cap_max=2 * N + 100, grow_rate=rate)


def _room(N, cfg):
    """The stride of a growth arena: seven pad rows behind the grown count."""
    from gaussiansplattingmlx_amd.mcmc import grown_count
    return grown_count(N, cfg.cap_max, cfg.grow_rate) + 7


# ------------------------------------------------------------------------------------------------------------- sizes
SIZES = [1, 3, 4, 5, TILE - 1, TILE, TILE + 1, 2 * TILE, 70_001]


@pytest.mark.parametrize("mode", [0, 1], ids=["relocate", "grow"])
@pytest.mark.parametrize("N", SIZES)
def test_sizes(renderer, N, mode):
    """A single block, a ragged one, exact multiples of the tile, one row more, 69 blocks; dead rows at the thread and block
    boundaries, a dead thread and a dead block (_placed).  At N = 1 the one row is dead: nothing to draw from, nothing relocated
    (test_one_live_row_alone is the other variant).  Growth doubles the small sizes (5 % of them adds nothing)."""
    p, dead = _scene(100 + N, N, extra_dead=600 if N > 50_000 else N // 20)
    cfg = _cfg(N, rate=1.0 if N <= 5 else 0.05)
    _, res, _ = _run(renderer, p, mode, cfg, 600 + mode, 1000 * N, stride=None if mode == 0 else _room(N, cfg), placed=dead)
    if mode == 0:
        assert res["dead"] == dead.size >= 1 and res["relocated"] == (dead.size if N > 1 else 0)
    else:
        assert res == (2 * N if N <= 5 else int(1.05 * N))


@pytest.mark.parametrize("mode", [0, 1], ids=["relocate", "grow"])
def test_one_live_row_alone(renderer, mode):
    """N = 1, the row live: no dead row, nothing relocated; the growth appends its copy (n = 2)."""
    p = _rows(7, 1)
    cfg = _cfg(1, rate=1.0)
    _, res, _ = _run(renderer, p, mode, cfg, 600, 40, stride=None if mode == 0 else 4)
    assert res == (dict(dead=0, relocated=0, live=1, N=1) if mode == 0 else 2)


# ------------------------------------------------------------------------------------------------------------- widths
@pytest.mark.parametrize("mode", [0, 1], ids=["relocate", "grow"])
@pytest.mark.parametrize("K", [1, 4, 9, 25])
def test_row_widths(renderer, K, mode):
    """The copy kernel's decode of element e of a row of F = 14 + 3 (K - 1) floats (K = 1: no features_rest at all), every
    float of a row distinct."""
    N = TILE + 1
    p, dead = _scene(200 + K, N, K, extra_dead=60)
    assert p["features_rest"].shape == (N, K - 1, 3)
    cfg = _cfg(N, rate=0.3)
    e, _, _ = _run(renderer, p, mode, cfg, 610 + mode, 7000 + K, stride=None if mode == 0 else _room(N, cfg), placed=dead)
    assert e["sources"].size == (dead.size if mode == 0 else int(1.3 * N) - N)


# ------------------------------------------------------------------------------------------------------------- the clamp
@pytest.mark.parametrize("mode", [0, 1], ids=["relocate", "grow"])
def test_n_is_clamped_on_the_device(renderer, mode):
    """One row at raw +8 among 499 at raw -5.0 (o = 0.0067) and 1500 dead ones: it holds about 23 % of the weight, so about 345
    of the 1500 draws (460 of the growth's 2000): n = min(c + 1, 51) = 51, the formula's longest sum."""
    from gaussiansplattingmlx_amd.mcmc import relocation_formula
    N = 2000
    p = _rows(31, N)
    p["opacity"][:] = -10.0
    weak = np.random.default_rng(32).choice(N, 500, replace=False)
    p["opacity"][weak] = -5.0
    top = int(weak[0])
    p["opacity"][top] = 8.0
    cfg = _cfg(N, rate=1.0)

    def drawn_52_times(e):
        assert e["counts"][top] >= 52, e["counts"][top]
        assert mode == 1 or e["stats"] == dict(dead=1500, relocated=1500, live=500, N=N)
    e, res, gv = _run(renderer, p, mode, cfg, 620, 300, stride=None if mode == 0 else 2 * N, host_check=drawn_52_times)
    on, ratio = relocation_formula(mn.sigmoid(np.float32(8.0)), 51, cfg.min_opacity, 51)          # the n = 51 values
    assert _ulps(gv["opacity"][top], np.float32(np.log(on / (1 - on)))) <= 1
    assert (_ulps(gv["scales"][top], np.log(np.exp(p["scales"][top].astype(np.float64)) * ratio).astype(np.float32)) <= 1).all()
    on52, _ = relocation_formula(mn.sigmoid(np.float32(8.0)), 52, cfg.min_opacity, 52)               # (and not the next n's)
    assert _ulps(gv["opacity"][top], np.float32(np.log(on52 / (1 - on52)))) > 1000


@pytest.mark.parametrize("mode", [0, 1], ids=["relocate", "grow"])
def test_a_single_live_row_takes_every_draw(renderer, mode):
    """Row 1024 live, the other 1499 dead: all 1499 relocation draws are its (the growth's 1500 but those that the dead rows'
    small weights win)."""
    N = 1500
    p = _rows(33, N)
    p["opacity"][:] = np.random.default_rng(34).uniform(-14, -9, N).astype(np.float32)
    p["opacity"][TILE] = 2.0
    cfg = _cfg(N, rate=1.0)
    e, res, _ = _run(renderer, p, mode, cfg, 630, 500, stride=None if mode == 0 else 2 * N)
    assert e["counts"][TILE] >= (N - 1 if mode == 0 else 52)
    if mode == 0:
        assert res == dict(dead=N - 1, relocated=N - 1, live=1, N=N)


def test_more_dead_rows_than_live_ones(renderer):
    N = 1000
    p = _rows(35, N)
    rng = np.random.default_rng(36)
    p["opacity"][:] = rng.uniform(-14, -6, N).astype(np.float32)
    live = np.sort(rng.choice(N, 100, replace=False))
    p["opacity"][live] = rng.uniform(-4, 3, 100).astype(np.float32)
    e, res, _ = _run(renderer, p, 0, _cfg(N), 640, 600)
    assert res == dict(dead=900, relocated=900, live=100, N=N) and np.isin(e["sources"], live).all()


# ------------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("mode", [0, 1], ids=["relocate", "grow"])
def test_non_finite_opacities(renderer, mode):
    """NaN (two payloads), +inf and -inf next to the thread and block boundaries among live rows: the relocation counts them
    dead and refills them, the growth gives them no weight and leaves them as they are, payload and all."""
    N = 2 * TILE + 452
    p, _ = _scene(41, N, extra_dead=0)
    p["opacity"][:] = np.random.default_rng(42).uniform(-4, 3, N).astype(np.float32)
    nan_a, nan_b = np.array([NAN_A, NAN_B], np.uint32).view(np.float32)
    odd = {3: nan_a, 4: np.inf, 8: -np.inf, 9: nan_b, 10: np.inf, 11: nan_a, TILE - 1: -np.inf, TILE: nan_a, TILE + 1: np.inf,
           2 * TILE - 1: nan_b, 2 * TILE: -np.inf, N - 1: np.inf, 0: nan_b}
    for i, x in odd.items():
        p["opacity"][i] = x
    rows = np.array(sorted(odd), np.int64)
    assert not np.isfinite(p["opacity"][rows]).any() and np.isfinite(np.delete(p["opacity"], rows)).all()
    assert _bits(p["opacity"][[3, 9]]).tolist() == [NAN_A, NAN_B]
    cfg = _cfg(N, rate=0.25)
    e, res, _ = _run(renderer, p, mode, cfg, 650 + mode, 800, stride=None if mode == 0 else _room(N, cfg))
    if mode == 0:
        assert res["dead"] == rows.size == res["relocated"] and np.array_equal(e["dests"], rows)
        assert np.isfinite(e["p"]["opacity"]).all()
    else:
        assert res == int(1.25 * N) and not np.isin(e["sources"], rows).any()
        assert np.array_equal(_bits(e["p"]["opacity"][rows]), _bits(p["opacity"][rows]))


# ------------------------------------------------------------------------------------------------------------- layouts
def test_relocation_on_a_strided_arena(renderer):
    """N = 1025 at 1500 rows per tensor: every moment offset is the strided layout's, and the 475 pad rows of every tensor and
    of its moments keep their (random) floats."""
    N = TILE + 1
    p, dead = _scene(51, N, extra_dead=80)
    _, res, _ = _run(renderer, p, 0, _cfg(N), 660, 900, stride=1500, placed=dead)
    assert res["relocated"] == dead.size


def test_growth_fills_the_capacity_exactly(renderer):
    """grow_rate = 1: N draws (the scratch of <= N draws full to its last word) into a stride of exactly 2 N rows."""
    N = TILE + 1
    p, _ = _scene(52, N, extra_dead=50)
    cfg = _cfg(N, rate=1.0)
    e, res, _ = _run(renderer, p, 1, cfg, 670, 1000, stride=2 * N)
    assert res == 2 * N and e["sources"].size == N


def test_growth_that_adds_nothing(renderer):
    """floor(1.05 * 10) = 10, and a cap_max at N: the count stays and nothing is written."""
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    p, _ = _scene(53, 10)
    for cfg in (_cfg(10), MCMCConfig(cap_max=10, grow_rate=1.0), MCMCConfig(cap_max=5, grow_rate=1.0)):
        model = _arena(p, 40)
        before = _flat(model)
        assert _call(renderer, model, 1, cfg.params(680, 3)) == 10
        for a, b, what in zip(_flat(model), before, ("parameters", "m", "v")):
            _same_bits(a, b, what)


def test_growth_stops_at_cap_max(renderer):
    """cap_max = 1050 between N = 1025 and floor(1.05 N) = 1076: 25 rows are added."""
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    N = TILE + 1
    p, _ = _scene(54, N, extra_dead=50)
    e, res, _ = _run(renderer, p, 1, MCMCConfig(cap_max=1050), 690, 1100, stride=1100)
    assert res == 1050 and e["sources"].size == 25


def test_growth_one_row_short_of_capacity_is_refused(renderer):
    """1076 rows into tensors of 1075: GS_ERR_SIZE_MISMATCH, nothing written, and the context takes the next event."""
    from gaussiansplattingmlx_amd._lib import GsplatError
    N = TILE + 1
    p, dead = _scene(55, N, extra_dead=50)
    cfg = _cfg(N)
    model = _arena(p, 1075)
    before = _flat(model)
    with pytest.raises(GsplatError) as err:
        _call(renderer, model, 1, cfg.params(700, 3))
    assert err.value.code == 2                                    # GS_ERR_SIZE_MISMATCH
    for a, b, what in zip(_flat(model), before, ("parameters", "m", "v")):
        _same_bits(a, b, what)
    _, res, _ = _run(renderer, p, 1, cfg, 700, 1200, stride=1076, repeat=False)
    assert res == 1076
    _run(renderer, p, 0, cfg, 700, 1200, stride=1075, repeat=False, placed=dead)


# ------------------------------------------------------------------------------------------------------------- scratch
def test_scratch_reuse_large_small_large():
    """One context of its own: both events at N = 70 001, then at 5, then at 70 001 again with other rows and another seed.  The
    scratch is grown once and kept; the per-source counts are cleared for the N words of the event at hand."""
    _gpu()
    from gaussiansplattingmlx_amd.renderer import GaussianRenderer
    r = GaussianRenderer(4, 160, 120, (16, 16), False)
    for i, N in enumerate((70_001, 5, 70_001)):
        p, dead = _scene(300 + i, N, extra_dead=500 if N > 5 else 0)
        for mode in (0, 1):
            cfg = _cfg(N, rate=1.0 if N == 5 else 0.05)
            _run(r, p, mode, cfg, 710 + i, 5000 * (i + 1), stride=None if mode == 0 else _room(N, cfg), repeat=False, placed=dead)


# ------------------------------------------------------------------------------------------------------------- refusals
def _raw_call(r, model, mode, prm, K=None, base_shift=0):
    """gs_mcmc_relocate / gs_mcmc_grow with a K or a param_base of the caller's choice: the status."""
    from gaussiansplattingmlx_amd.renderer import _p
    Kt, t = r._mcmc_rows(model.getParams())
    base = C.c_void_p(model.arena.data_ptr() + base_shift)
    tail = (base, _p(model.m), _p(model.v), C.byref(prm))
    if mode == 0:
        return r.lib.gs_mcmc_relocate(r.ctx, model.N, Kt if K is None else K, *t, *tail, (C.c_longlong * 4)())
    n = C.c_int(-1)
    return r.lib.gs_mcmc_grow(r.ctx, model.N, model.stride, Kt if K is None else K, *t, *tail, C.byref(n))


@pytest.mark.parametrize("mode", [0, 1], ids=["relocate", "grow"])
@pytest.mark.parametrize("what", ["K=0", "K=26", "below_param_base", "n_max=52", "grow_rate=1.5"])
def test_refusals_write_nothing(renderer, what, mode):
    from gaussiansplattingmlx_amd.mcmc import MCMCConfig
    N = 300
    p, _ = _scene(61, N, extra_dead=40)
    model = _arena(p, 2 * N)
    before = _flat(model)
    good = MCMCConfig(cap_max=2 * N, grow_rate=1.0)
    cfg = {"n_max=52": MCMCConfig(cap_max=2 * N, grow_rate=1.0, n_max=52),
           "grow_rate=1.5": MCMCConfig(cap_max=2 * N, grow_rate=1.5)}.get(what, good)
    kw = {"K=0": dict(K=0), "K=26": dict(K=26), "below_param_base": dict(base_shift=16)}.get(what, {})
    rc = _raw_call(renderer, model, mode, cfg.params(720, 3), **kw)
    assert rc == 1, rc                                            # GS_ERR_INVALID_ARG
    torch.cuda.synchronize()
    for a, b, name in zip(_flat(model), before, ("parameters", "m", "v")):
        _same_bits(a, b, name)
    assert _raw_call(renderer, model, mode, good.params(720, 3)) == 0           # (and the same call, unspoiled, runs)
