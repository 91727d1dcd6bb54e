"""The MCMC strategy without a device: the float64 relocation formula, MCMCConfig's validation, the trainer's refusals and the
generator's restatement (tests/mcmc_numpy.py)."""
import decimal
import importlib.util
import math
import os

import numpy as np
import pytest

from gaussiansplattingmlx_amd.mcmc import MCMCConfig, grown_count, relocation_formula

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_mcmc_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mn = _load("mcmc_numpy")
O = np.array([1e-3, 0.005, 0.02, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999])


def test_n1_is_the_identity():
    on, ratio = relocation_formula(O, 1, min_opacity=1e-4)
    np.testing.assert_allclose(on, O, rtol=1e-14, atol=0)
    np.testing.assert_allclose(ratio, 1.0, rtol=1e-14)


@pytest.mark.parametrize("n", [2, 3, 5, 10, 25, 51])
def test_n_copies_compose_the_opacity(n):
    on, _ = relocation_formula(O, n, min_opacity=1e-12)
    keep = (on > 1e-12) & (on < 1 - 2.0 ** -23)        # (outside the clamp)
    np.testing.assert_allclose((1 - (1 - on) ** n)[keep], O[keep], rtol=0, atol=1e-12)


def test_n2_closed_form():
    on, ratio = relocation_formula(O, 2, min_opacity=1e-12)
    np.testing.assert_allclose(ratio, O / (2 * on - on * on / math.sqrt(2)), rtol=1e-12)


def test_n_is_clamped_at_n_max():
    a = relocation_formula(O, 200, n_max=51)
    b = relocation_formula(O, 51, n_max=51)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    c = relocation_formula(O, 9, n_max=4)
    d = relocation_formula(O, 4, n_max=51)
    np.testing.assert_array_equal(c[1], d[1])


def test_clamp_bounds():
    on, _ = relocation_formula(np.array([1e-6, 1.0 - 1e-12]), 1, min_opacity=0.005)
    assert on[0] == 0.005 and on[1] == 1.0 - 2.0 ** -23


def _formula_decimal(o: float, n: int, min_opacity: float, digits: int = 60):
    """relocation_formula's expression for one float64 o at `digits` decimal digits: the n-th root through ln / exp."""
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        o = D(o)                                                    # (a float converts exactly)
        on = 1 - ((1 - o).ln() / n).exp()
        on = min(max(on, D(min_opacity)), 1 - D(2) ** -23)
        den = D(0)
        for a in range(1, n + 1):
            pw = on
            for k in range(a):
                term = math.comb(a - 1, k) * pw / D(k + 1).sqrt()
                den += -term if k & 1 else term
                pw *= on
        return on, o / den


RAW = np.concatenate([np.linspace(-5.2, 30.0, 45), [-5.0, -1.0, 0.0, 1.0, 8.0, 17.3, 29.9]]).astype(np.float32)


@pytest.mark.parametrize("n", [2, 3, 5, 10, 20, 35, 51])
def test_formula_against_60_digit_decimal(n):
    """The float64 formula against the same expression at 60 digits, raw opacities in [-5.2, 30] (the lower
    clamp of o' included): 1e-9 relative on both results, about five times what float64 reaches here (2.4e-10, n = 51).
    The range ends below raw = 37, where sigmoid(raw) rounds to 1.0 in float64 (relocation_formula's docstring)."""
    o = mn.sigmoid(RAW)
    assert RAW.min() == np.float32(-5.2) and RAW.max() == 30.0 and (o < 1.0).all()
    on, ratio = relocation_formula(o, n, 0.005, 51)
    worst = 0.0
    for i in range(o.size):
        won, wr = _formula_decimal(float(o[i]), n, 0.005)
        for got, want in ((on[i], won), (ratio[i], wr)):
            worst = max(worst, float(abs(decimal.Decimal(float(got)) - want) / abs(want)))
    print(f"n={n}: worst relative error {worst:.3e}")
    assert worst <= 1e-9, worst


def _three_rows(raw, K=2):
    """Three hand-made rows of distinct floats (row i's values start at 100 i), their moments nonzero everywhere."""
    N = len(raw)
    shapes = dict(xyz=(3,), features_dc=(1, 3), features_rest=(K - 1, 3), scales=(3,), rotation=(4,), opacity=())
    p, off = {}, 1.0
    for k in mn.KEYS:
        per = int(np.prod(shapes[k])) if shapes[k] else 1
        p[k] = (off + 100.0 * np.arange(N)[:, None] + np.arange(per)[None, :]).reshape((N,) + shapes[k]).astype(np.float32)
        off += per
    p["scales"] = (p["scales"] * np.float32(1e-2) - 3).astype(np.float32)
    p["opacity"] = np.asarray(raw, np.float32)
    m = {k: (np.zeros_like(p[k]) + 0.25 + np.arange(N).reshape((N,) + (1,) * (p[k].ndim - 1))).astype(np.float32) for k in mn.KEYS}
    v = {k: (m[k] + 7).astype(np.float32) for k in mn.KEYS}
    return p, m, v


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_event_three_rows_one_dead():
    """Rows 0 and 1 live (o = 0.5, 0.731), row 2 dead: one draw u, the source is row 0 iff u (o0 + o1) < o0; n = 2, whose
    formula has the closed form o' = 1 - sqrt(1 - o), s'/s = o / (2 o' - o'^2 / sqrt 2)."""
    cfg, t, seed = MCMCConfig(), 600, 12345
    p, m, v = _three_rows([0.0, 1.0, -10.0])
    e = mn.event(p, m, v, 0, cfg, t, seed)
    o = mn.sigmoid(p["opacity"])
    u = mn.uniforms(mn.philox([0], t, 1, seed))[0]
    s = 0 if u * (o[0] + o[1]) < o[0] else 1
    other = 1 - s
    assert e["stats"] == dict(dead=1, relocated=1, live=2, N=3) and e["N"] == 3
    assert e["sources"].tolist() == [s] and e["dests"].tolist() == [2] and e["counts"].tolist() == [1 - s, s, 0]
    on = 1 - math.sqrt(1 - o[s])
    ratio = o[s] / (2 * on - on * on / math.sqrt(2))
    np.testing.assert_allclose(e["p"]["opacity"][s], math.log(on / (1 - on)), rtol=2e-7)
    np.testing.assert_allclose(e["p"]["scales"][s], p["scales"][s].astype(np.float64) + math.log(ratio), rtol=2e-7)
    for k in mn.KEYS:
        assert e["p"][k].dtype == np.float32 and e["p"][k].shape == p[k].shape
        assert np.array_equal(_bits(e["p"][k][2]), _bits(e["p"][k][s])), k                # the destination: the modified source
        if k not in ("opacity", "scales"):
            assert np.array_equal(_bits(e["p"][k][s]), _bits(p[k][s])), k                 # the source keeps everything else
        assert np.array_equal(_bits(e["p"][k][other]), _bits(p[k][other])), k             # the row not drawn: untouched
        for got, was in ((e["m"][k], m[k]), (e["v"][k], v[k])):
            assert (got[[s, 2]] == 0).all() and np.array_equal(_bits(got[other]), _bits(was[other])), k
    assert p["opacity"][2] == np.float32(-10.0) and (m["xyz"] != 0).all()                # the inputs are left alone


@pytest.mark.parametrize("raw", [[-10.0, -9.0, -8.0], [np.nan, np.inf, -np.inf]])
def test_event_every_row_dead(raw):
    cfg = MCMCConfig(cap_max=100, grow_rate=1.0)
    p, m, v = _three_rows(raw)
    p["xyz"][1, 0] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]               # a NaN payload survives
    e = mn.event(p, m, v, 0, cfg, 600, 7)
    assert e["stats"] == dict(dead=3, relocated=0, live=0, N=3) and e["sources"].size == 0
    g = mn.event(p, m, v, 1, cfg, 600, 7)              # growth: finite rows keep their weight, non-finite ones have none
    assert g["N"] == (6 if np.isfinite(raw).all() else 3)
    for out in (e, g) if g["N"] == 3 else (e,):
        for k in mn.KEYS:
            for got, was in ((out["p"][k], p[k]), (out["m"][k], m[k]), (out["v"][k], v[k])):
                assert np.array_equal(_bits(got), _bits(was)), k


def test_event_no_row_dead():
    cfg = MCMCConfig(cap_max=100)
    p, m, v = _three_rows([0.0, 1.0, 2.0])
    e = mn.event(p, m, v, 0, cfg, 600, 7)
    assert e["stats"] == dict(dead=0, relocated=0, live=3, N=3)
    for k in mn.KEYS:
        for got, was in ((e["p"][k], p[k]), (e["m"][k], m[k]), (e["v"][k], v[k])):
            assert np.array_equal(_bits(got), _bits(was)), k
    assert mn.event(p, m, v, 1, cfg, 700, 7)["N"] == 3                 # floor(1.05 * 3) = 3: nothing to add
    # growth by two rows: rows 3 and 4 are copies of their modified sources, n = draws + 1 on every source
    g = mn.event(p, m, v, 1, cfg, 700, 7, n_add=2)
    o = mn.sigmoid(p["opacity"])
    u = mn.uniforms(mn.philox([0, 1], 700, 2, 7))
    src = np.searchsorted(np.cumsum(o), u * o.sum(), side="right")
    assert g["N"] == 5 and g["stats"] is None and g["sources"].tolist() == src.tolist() and g["dests"].tolist() == [3, 4]
    cnt = np.bincount(src, minlength=3)
    on, ratio = relocation_formula(o, cnt + 1, cfg.min_opacity, cfg.n_max)
    for i in range(3):
        if cnt[i]:
            np.testing.assert_allclose(mn.sigmoid(g["p"]["opacity"][i]), on[i], rtol=1e-6)
            np.testing.assert_allclose(np.exp(g["p"]["scales"][i].astype(np.float64)),
                                       np.exp(p["scales"][i].astype(np.float64)) * ratio[i], rtol=1e-6)
        else:
            assert g["p"]["opacity"][i] == p["opacity"][i] and np.array_equal(g["p"]["scales"][i], p["scales"][i])
    for k in mn.KEYS:
        assert g["p"][k].shape == (5,) + p[k].shape[1:]
        for j in range(2):
            assert np.array_equal(_bits(g["p"][k][3 + j]), _bits(g["p"][k][src[j]])), k
        for got, was in ((g["m"][k], m[k]), (g["v"][k], v[k])):
            assert (got[3:] == 0).all() and (got[:3][cnt > 0] == 0).all()
            assert np.array_equal(_bits(got[:3][cnt == 0]), _bits(was[cnt == 0])), k


def test_min_boundary_gap():
    cdf = np.array([1.0, 3.0, 4.0])
    assert mn.min_boundary_gap(cdf, [0.5, 2.0]) == 0.125           # 0.5 from the entry 1.0, of a total of 4
    assert mn.min_boundary_gap(cdf, [3.0 + 4e-9]) == pytest.approx(1e-9, rel=1e-6)
    assert mn.min_boundary_gap(cdf, [3.9]) == pytest.approx(0.025)
    assert mn.min_boundary_gap(cdf, []) == np.inf


def test_grown_count():
    assert grown_count(300_000, 1_000_000, 0.05) == 315_000
    assert grown_count(990_000, 1_000_000, 0.05) == 1_000_000
    assert grown_count(1_000_000, 1_000_000, 0.05) == 1_000_000
    assert grown_count(10, 100, 0.05) == 10            # floor(10.5) = 10: nothing to add
    assert grown_count(21, 100, 0.05) == 22


def test_config_defaults_are_gsplats():
    c = MCMCConfig()
    assert (c.cap_max, c.noise_lr, c.opacity_reg, c.scale_reg, c.min_opacity, c.refine_start, c.refine_stop, c.refine_every,
            c.grow_rate, c.n_max, c.seed) == (1_000_000, 5e5, 0.01, 0.01, 0.005, 500, 25_000, 100, 0.05, 51, None)
    assert c.validate() is c


@pytest.mark.parametrize("field,value", [("cap_max", 0), ("cap_max", 1.5), ("noise_lr", -1.0), ("noise_lr", float("nan")),
                                         ("opacity_reg", float("inf")), ("scale_reg", -0.1), ("min_opacity", 0.0),
                                         ("min_opacity", 1.0), ("grow_rate", -0.01), ("grow_rate", 1.5), ("n_max", 0),
                                         ("n_max", 52), ("refine_every", 0), ("refine_start", -1), ("seed", -1),
                                         ("seed", 2 ** 64), ("n_max", True)])
def test_config_validation_refuses(field, value):
    with pytest.raises(ValueError):
        MCMCConfig(**{field: value}).validate()


def test_event_cadence():
    c = MCMCConfig()
    ev = [t for t in range(30_000) if c.is_event(t)]
    assert ev[0] == 600 and ev[-1] == 24_900 and len(ev) == 244     # 500 < t < 25000, every 100 steps
    assert MCMCConfig(refine_start=0, refine_stop=10, refine_every=3).is_event(9)


def test_params_struct():
    p = MCMCConfig(cap_max=1234, seed=None).params(77, 2 ** 63 + 5)
    assert p.cap_max == 1234 and p.iteration == 77 and p.seed == 2 ** 63 + 5 and p.n_max == 51
    assert MCMCConfig(seed=9).params(0, 123).seed == 9


class _Model:
    N, capacity = 100, 100


def _trainer(**kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    return GaussianTrainer(_Model(), None, **kw)


@pytest.mark.parametrize("kw", [dict(strategy="nope"), dict(mcmc=MCMCConfig()), dict(strategy="mcmc", mcmc=dict(cap_max=5)),
                                dict(strategy="mcmc", mcmc=MCMCConfig(cap_max=99)),
                                dict(strategy="mcmc", mcmc=MCMCConfig(n_max=0)),
                                dict(strategy="mcmc", process_group=object()),
                                dict(strategy="mcmc", dp_bootstrap=(b"", 0, 1), exchange_impl="native"),
                                dict(strategy="mcmc", exchange_impl="native"),
                                dict(strategy="mcmc", views_per_rank=2)])
def test_trainer_refusals_without_a_device(kw):
    """Refused before the trainer touches the renderer or the model's buffers."""
    with pytest.raises(ValueError):
        _trainer(**kw)


def test_reference_param_reload_is_refused_under_mcmc():
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    tr = GaussianTrainer.__new__(GaussianTrainer)
    tr.mcmc = MCMCConfig()
    with pytest.raises(ValueError):
        tr.referenceParamReload = True
    tr.referenceParamReload = False
    tr.mcmc = None
    tr.referenceParamReload = True
    assert tr.referenceParamReload


def test_philox_known_answer():
    """The restatement against the Random123 known-answer vectors of Philox4x32-10 (counter / key all zero, all ones):
    the same rounds as csrc/gs_mcmc.h with the counter fields set directly."""
    def raw(c, k):
        c = [np.uint64(x) for x in c]
        k0, k1 = np.uint64(k[0]), np.uint64(k[1])
        for _ in range(10):
            p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
            c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mn.M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mn.M32]
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mn.M32, (k1 + np.uint64(0xBB67AE85)) & mn.M32
        return [int(x) for x in c]
    assert raw([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    m = 0xFFFFFFFF
    assert raw([m, m, m, m], [m, m]) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    w = mn.philox(np.arange(3), 5, 0, 77)
    assert w.shape == (3, 4) and w.dtype == np.uint32 and len({tuple(r) for r in w}) == 3


def test_restated_draws_follow_the_weights():
    rng = np.random.default_rng(3)
    raw = rng.normal(0, 2, 5000).astype(np.float32)
    raw[:500] = -12.0
    raw[10] = np.nan
    src, target, cdf, rows, dead = mn.draw(raw, 0, 0.005, 200_000, 20260313, 700)
    assert set(dead.tolist()) >= set(range(500)) and 10 in dead.tolist()
    assert np.isin(src, rows).all()
    o = mn.sigmoid(raw[rows])
    freq = np.bincount(np.searchsorted(rows, src), minlength=len(rows)) / len(src)
    assert np.abs(freq - o / o.sum()).max() < 5e-4
