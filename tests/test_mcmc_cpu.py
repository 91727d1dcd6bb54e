"""The MCMC strategy without a device: the float64 relocation formula, MCMCConfig's validation, the trainer's refusals and the
generator's restatement (tests/mcmc_numpy.py)."""
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
