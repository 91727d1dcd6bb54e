"""Qualifies tests/densify_numpy.py, the restatement tests/test_gpu_densify_kernels.py holds csrc/densify.hip to, without a
device: the generic Philox4x32-10 against the Random123 known answers and against the MCMC generator's restatement, the scan
and the output map against the C oracle on every action mix and size the GPU file uses, the float32 walk of the noise against
its float64 form (it may use half of the GPU test's bar), and the classify inputs against the exclusion rule's cap."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_dncpu_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dz = _load("densify_numpy")
mn = _load("mcmc_numpy")


def test_philox_meets_the_known_answers():
    """The two Random123 vectors tests/test_mcmc_cpu.py::test_philox_known_answer holds the MCMC restatement to."""
    m = 0xFFFFFFFF
    got = dz.philox4x32_10([[0, 0, 0, 0], [m, m, m, m]], (0, 0))
    assert got[0].tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    got = dz.philox4x32_10([[m, m, m, m]], (m, m))
    assert got[0].tolist() == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.mark.parametrize("stream", [0, 1, 2])
def test_philox_reproduces_the_mcmc_generator(stream):
    n, t, seed = 4096, 700 + stream, 0x1234_5678_9ABC_DEF0
    c = np.zeros((n, 4), np.uint64)
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = np.arange(n), t, mn.TAG0, mn.TAGS[stream]
    got = dz.philox4x32_10(c, (seed & 0xFFFFFFFF, seed >> 32))
    np.testing.assert_array_equal(got, mn.philox(np.arange(n), t, stream, seed))


def test_noise_counter_and_key():
    """densify_noise3's counter is (row, 0, 0x64656e73, 0x69667921) under the key (seed low, seed high), and a row's words do
    not depend on how many rows are asked for."""
    seed = 2 ** 64 - 1
    w = dz.noise_words(seed, 300)
    c = np.zeros((300, 4), np.uint64)
    c[:, 0], c[:, 2], c[:, 3] = np.arange(300), 0x64656E73, 0x69667921
    np.testing.assert_array_equal(w, dz.philox4x32_10(c, (0xFFFFFFFF, 0xFFFFFFFF)))
    np.testing.assert_array_equal(dz.noise_words(seed, np.array([299, 7])), w[[299, 7]])
    assert not np.array_equal(dz.noise_words(2 ** 32, 4), dz.noise_words(1, 4))       # (the high half is the second key word)


def test_noise_uniforms_round_as_float32_does():
    """The uniform's float32 sum rounds to even from w >> 8 = 2^23 on, u = 1 occurs and gives a radius of exactly zero."""
    w = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0x80000100] * 4, [0x80000000] * 4], np.uint32)
    u, ang = dz.noise_uniforms(w)
    assert u[0, 0] == np.float32(0.5 / 16777216.0) and u[1, 0] == np.float32(1.0)
    assert u[2, 0] == np.float32((2 ** 23 + 2) / 16777216.0)          # 2^23 + 1 + 1/2 rounds to the even 2^23 + 2
    assert u[3, 0] == np.float32(2 ** 23 / 16777216.0)                # 2^23 + 1/2 rounds to the even 2^23
    assert ang[1, 0] == np.float32(6.2831855)
    for dtype in (np.float64, np.float32):
        ra = np.sqrt(dtype(-2.0) * np.log(u[:, 0].astype(dtype)))
        assert ra[1] == 0.0 and np.isfinite(ra).all()


def test_float32_walk_of_the_noise_stays_within_half_the_bar():
    worst = 0.0
    for seed in dz.NOISE_SEEDS:
        z64 = dz.densify_noise(seed, max(dz.NOISE_ROWS))
        z32 = dz.densify_noise(seed, max(dz.NOISE_ROWS), np.float32)
        assert z64.dtype == np.float64 and z32.dtype == np.float32 and np.isfinite(z64).all()
        worst = max(worst, float(np.abs(z32.astype(np.float64) - z64).max()))
        z = z64
        assert abs(z.mean()) < 0.05 and abs(z.std() - 1) < 0.05 and np.abs(z).max() < 6.5
    print("densify noise, float32 walk vs float64: worst", worst)
    assert worst <= 0.5 * dz.NOISE_BAR, worst


@pytest.mark.parametrize("N", dz.SCAN_NS)
def test_scan_and_map_equal_the_oracle(oracle32, N):
    for mix in dz.MIXES + ("prune_only",):
        a = dz.actions_of(mix, N)
        c = dz.counts_of(a)
        assert a.dtype == np.int32 and c.dtype == np.int32 and a.shape == (N,)
        woff, wst = oracle32.densify_offsets(a, c)
        off, st = dz.offsets(a)
        assert st == wst, (mix, st, wst)
        np.testing.assert_array_equal(off, woff, err_msg=mix)
        wg, wm = oracle32.build_densify_output_map(a, woff, wst["total"])
        g, m = dz.output_map(a, off, st["total"])
        np.testing.assert_array_equal(g, wg, err_msg=mix)
        np.testing.assert_array_equal(m, wm, err_msg=mix)
        words = dz.plan(a, N)
        applies = st["total"] > 0 and (st["split"] + st["clone"] + st["prune"]) > 0
        assert words == [st["total"] if applies else N, int(applies), st["total"], st["keep"], st["split"], st["clone"],
                         st["prune"], N]


def test_the_mixes_are_what_their_names_say():
    N = 2 * dz.SCAN_CHUNK + 1
    assert abs(np.bincount(dz.actions_of("random", N), minlength=4) / N - [0.7, 0.1, 0.1, 0.1]).max() < 0.01
    a = dz.actions_of("chunk0_prune", N)
    assert (a[:dz.SCAN_CHUNK] == 3).all() and len(np.unique(a[dz.SCAN_CHUNK:])) == 4
    a = dz.actions_of("alternating_tiles", 4097)
    assert (a[:1024] == 3).all() and (a[1024:2048] == 1).all() and (a[2048:3072] == 3).all() and a[4096] == 3
    for mix, row, act in (("first_split", 0, 1), ("first_prune", 0, 3), ("last_split", 1024, 1), ("last_prune", 1024, 3)):
        a = dz.actions_of(mix, 1025)
        assert a[row] == act and np.count_nonzero(a) == 1
    a = dz.actions_of("prune_only", 1000)
    assert set(np.unique(a)) == {0, 3}
    assert dz.plan(dz.actions_of("all_prune", 77), 77) == [77, 0, 0, 0, 0, 0, 77, 77]
    assert dz.plan(dz.actions_of("all_keep", 77), 77) == [77, 0, 77, 77, 0, 0, 0, 77]


def test_maps_that_do_not_fit_and_the_planned_forms():
    """A row whose slots do not fit `total` writes nothing (build_map_kernel); the planned map clamps total to the capacity and
    is the identity below min(N, capacity) when nothing applies."""
    a = np.array([0, 1, 3, 2, 0, 3, 1], np.int32)                 # tests/test_densify_oracle.py's hand-worked case
    off, st = dz.offsets(a)
    assert off.tolist() == [0, 1, 3, 3, 5, 6, 6] and st == dict(total=8, keep=2, split=2, clone=1, prune=2)
    g, m = dz.output_map(a, off, 8)
    assert g.tolist() == [0, 1, 1, 3, 3, 4, 6, 6] and m.tolist() == [0, 1, 2, 0, 3, 0, 1, 2]
    g, m = dz.output_map(a, off, 7)                                # the last split needs slots 6 and 7: it writes neither
    assert g.tolist() == [0, 1, 1, 3, 3, 4, 0] and m.tolist() == [0, 1, 2, 0, 3, 0, 0]
    words = dz.plan(a, 7)
    assert words == [8, 1, 8, 2, 2, 1, 2, 7]
    g, m = dz.planned_map(a, off, words, 10)
    assert g.tolist() == [0, 1, 1, 3, 3, 4, 6, 6, 0, 0] and m.tolist() == [0, 1, 2, 0, 3, 0, 1, 2, 0, 0]
    g, m = dz.planned_map(a, off, words, 4)                        # the clone needs slots 3 and 4
    assert g.tolist() == [0, 1, 1, 0] and m.tolist() == [0, 1, 2, 0]
    keep = np.zeros(5, np.int32)
    off, _ = dz.offsets(keep)
    for cap, want in ((4, [0, 1, 2, 3]), (5, [0, 1, 2, 3, 4]), (7, [0, 1, 2, 3, 4, 0, 0])):
        g, m = dz.planned_map(keep, off, dz.plan(keep, 5), cap)
        assert g.tolist() == want and not m.any()


@pytest.mark.parametrize("K", [1, 4])
def test_gather_equals_the_oracle(oracle32, oracle64, K):
    N = 257
    p = dz.gather_params(N, K)
    a = dz.actions_of("random", N)
    off, st = dz.offsets(a)
    g, m = dz.output_map(a, off, st["total"])
    nz = dz.densify_noise(7, st["total"]).astype(np.float32)
    got = dz.gather(p, g, m, nz)
    want32, want64 = oracle32.densify_gather(p, g, m, nz), oracle64.densify_gather(p, g, m, nz)
    for k in dz.PARAMS:
        if k != "xyz":
            np.testing.assert_array_equal(got[k].astype(np.float32), want32[k].reshape(got[k].shape), err_msg=k)
            # (float64 oracle: it reduces a split's scales by the double -log 1.6, the kernel by its float32 rounding)
            atol = abs(float(dz.SCALE_REDUCTION) + np.log(1.6)) + 1e-15 if k == "scales" else 0.0
            np.testing.assert_allclose(got[k], want64[k].reshape(got[k].shape), rtol=0, atol=atol, err_msg=k)
    # xyz: the restatement multiplies by the kernel's float32 constants 0.1f and 0.01f, the float64 oracle by 0.1 and 0.01 --
    # 1.5e-8 and 2.2e-8 apart -- and the mean by 1.0f / 3.0f, 3.0e-8 from 1 / 3: at most 4.5e-8 of the noise term alone
    moved = np.abs(got["xyz"] - p["xyz"][g])
    assert (np.abs(got["xyz"] - want64["xyz"]) <= 5e-8 * moved + 1e-15).all()
    assert np.abs(got["xyz"] - p["xyz"][g]).max() > 1e-4 and (got["scales"] != p["scales"][g]).any()
    plain = dz.gather(p, g, m, None)
    for k in dz.PARAMS:
        np.testing.assert_array_equal(plain[k], p[k][g], err_msg=k)


@pytest.mark.parametrize("th", dz.CLASSIFY_THRESHOLDS, ids=["default", "other"])
def test_classify_inputs_stay_under_the_exclusion_cap(oracle32, oracle64, th):
    """The hand-placed rows decide as intended on both oracles, column 3 of the [N, 4] scales is never read, and the rows the
    exclusion rule drops stay under the existing test's cap of 1e-3."""
    acc, scales, opacity = dz.classify_inputs(th)
    assert np.isfinite(acc).all() and not np.isnan(scales).any() and not np.isnan(opacity).any()
    near = dz.classify_near(th, scales, opacity)
    assert near.mean() < 1e-3 and not near[:48].any()
    for denom in dz.CLASSIFY_DENOMS:
        for allow in (True, False):
            a32, c32 = oracle32.classify_gaussians(acc, denom, scales, opacity, allowDensify=allow, **th)
            a64, c64 = oracle64.classify_gaussians(acc, denom, scales, opacity, allowDensify=allow, **th)
            # (rows 0 .. 23 sit at and one float32 ulp beside the FLOAT32 threshold: the float64 oracle's threshold is another number)
            np.testing.assert_array_equal(a32[24:][~near[24:]], a64[24:][~near[24:]])
            np.testing.assert_array_equal(c32, dz.counts_of(a32))
            a3, _ = oracle32.classify_gaussians(acc, denom, np.ascontiguousarray(scales[:, :3]), opacity, allowDensify=allow, **th)
            np.testing.assert_array_equal(a32, a3)
            if denom <= 0 or not allow:
                assert set(np.unique(a32)) <= {0, 3}
    a, _ = oracle32.classify_gaussians(acc, 8.0, scales, opacity, **th)
    assert a[0:8].tolist() == [0] * 8                              # exactly at the threshold: strict, keeps
    assert a[8:16].tolist() == [2, 1] * 4                          # one ulp above: clone (small) / split (large)
    assert a[16:24].tolist() == [0] * 8
    assert a[24:40].tolist() == [1, 3, 1, 3, 2, 3, 2, 3, 1, 3, 1, 3, 2, 3, 2, 3]      # exp(89) = inf splits, exp(-104) = 0 clones
    assert a[44:48].tolist() == [3] * 4 and 3 not in a[40:44].tolist()
    assert len(np.unique(a)) == 4


@pytest.mark.parametrize("N", dz.ACCUM_NS)
def test_accumulate_inputs_reach_the_underflow_and_the_overflow(oracle32, N):
    g, acc = dz.accum_inputs(N)
    out = oracle32.accum_grad_norm(g, acc)
    assert out[0] == acc[0]                                        # 1e-25 squared is zero in float32
    if N > 4:
        assert np.isinf(out[1]) and np.isinf(out[3]) and out[4] == acc[4] and np.isfinite(out[2]) and out[2] > acc[2]
    assert not np.isnan(out).any()
