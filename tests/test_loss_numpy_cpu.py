"""tests/loss_numpy.py on the CPU: the float64 statement of the training loss against Oracle(np.float64), the properties the
structured image pairs are there for, the cap that keeps the float32 oracle's own error -- the allowance of every bar -- from
swallowing a failure, and the sensitivity of images and bars to six deliberate mistakes.

Which pair rejects which mistake (through loss_numpy.bars, each mistake evaluated in float64 in place of the kernel, at each
of (45, 70), (33, 65), (97, 161) and (64, 96); test_mistakes_are_rejected asserts this list):
  border_clamped         every pair but flat_equal and white_equal, by loss, mean ssim and cotangent (a constant image clamped
                         at the border is the same constant, equal to its target as before)
  taps_centred           every pair but flat_equal and white_equal (both means move alike and the quotient stays 1); noise
                         and flat_vs_flat by the cotangent (almost) alone, the others by loss and mean ssim too
  sign_zero_negative     every pair that has equal pixels, by the cotangent, one whole unit u at each of them: flat_equal,
                         white_equal, white_bg, blobs_near, ramp, step_edge, saturated, zero_band at every shape
                         (blobs_vs_blobs too where both clip at 1 in the same place); it cannot act on the others
  target_stats_shifted   every pair, the equal ones too (near the left and right border a flat image's windowed statistics
                         depend on the column), by loss, mean ssim and cotangent
  ssim_mean_padded       every pair, by the mean ssim and the loss; at (64, 96), whole tiles, it cannot act and changes nothing
  backward_unflipped     every pair but flat_equal and white_equal (a zero upstream derivative has no orientation), by the
                         cotangent
The two equal pairs are in the set for sign(0), the cancellation in sigma and the zero of the cotangent."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_lncpu_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ln = _load("loss_numpy")
SHAPES = ln.SHAPES_ALL_PAIRS
WHOLE_TILES = (64, 96)
ZERO_COT = 1e-12                # in units of u: what counts as the zero cotangent of an equal pair in float64
ALL = tuple(ln.PAIRS)
NOT_EQUAL = tuple(n for n in ALL if n not in ln.EQUAL_PAIRS)
WITH_EQUAL_PIXELS = ("flat_equal", "white_equal", "white_bg", "blobs_near", "ramp", "step_edge", "saturated", "zero_band")
# the pairs that must reject each mistake at every shape where it can act (the docstring's matrix)
REJECTED_BY = dict(border_clamped=NOT_EQUAL, taps_centred=NOT_EQUAL, sign_zero_negative=WITH_EQUAL_PIXELS,
                   target_stats_shifted=ALL, ssim_mean_padded=ALL, backward_unflipped=NOT_EQUAL)


def test_window_is_the_oracles_bit_for_bit(oracle32):
    want = oracle32.ssim_window().reshape(ln.K, ln.K)
    got = ln.window()
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.float32), want) and np.array_equal(got, want.astype(np.float64))
    assert abs(float(ln.taps().sum()) - 1.0) < 1e-6 and not np.array_equal(ln.taps(), ln.taps()[::-1])     # off-centre: not symmetric


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("name", ALL)
def test_statement_is_the_float64_oracle(oracle32, oracle64, name, H, W):
    ref = ln.reference(oracle32, oracle64, name, H, W)
    got, want = ln.loss_statement(ref["render"], ref["target"]), ref["ref64"]
    for k in ("loss", "l1", "ssim"):
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    assert np.abs(got["cot"] - want["cot"]).max() <= 1e-12 * max(np.abs(want["cot"]).max(), ln.unit(want["cot"].shape))


@pytest.mark.parametrize("H,W", SHAPES)
def test_every_image_has_the_property_it_is_there_for(oracle32, oracle64, H, W):
    P = {n: ln.reference(oracle32, oracle64, n, H, W) for n in ALL}
    for n, ref in P.items():
        r, t = ref["render"], ref["target"]
        assert r.dtype == t.dtype == np.float32 and r.shape == t.shape == (H, W, 3) and np.isfinite(r).all() and np.isfinite(t).all()
        r2, t2 = ln.PAIRS[n](H, W, ln.SEED)
        assert np.array_equal(r, r2) and np.array_equal(t, t2), n                  # deterministic
    eq = {n: float((P[n]["render"] == P[n]["target"]).mean()) for n in ALL}
    out = {n: float(((P[n]["render"] < 0) | (P[n]["render"] > 1)).mean()) for n in ALL}
    # the equal pairs: equal everywhere, the exact constants, and a cotangent of zero.  (The float64 oracle's is up to 7e-15 u,
    # not 0.0: its up / den b and up num / den^2 d are equal in exact arithmetic only.  The statement's is held to the same.)
    for n, v in (("flat_equal", 0.5), ("white_equal", 1.0)):
        assert eq[n] == 1.0 and (P[n]["render"] == np.float32(v)).all()
        assert np.abs(P[n]["ref64"]["cot"]).max() <= ZERO_COT * ln.unit((H, W, 3)) and P[n]["ref64"]["l1"] == 0.0
        assert np.abs(ln.loss_statement(P[n]["render"], P[n]["target"])["cot"]).max() <= ZERO_COT * ln.unit((H, W, 3))
        assert abs(P[n]["ref64"]["ssim"] - 1.0) < 1e-12
    assert eq["flat_vs_flat"] == 0.0 and eq["noise"] == 0.0
    assert (P["zeros_vs_blobs"]["render"] == 0).all() and P["zeros_vs_blobs"]["target"].max() > 0.5
    # exact 1.0 background, and half of it equal in the target (the noise clipped)
    white = P["white_bg"]["render"] == 1.0
    assert white.mean() > 0.1 and 0.02 < eq["white_bg"] < white.mean()
    assert eq["saturated"] >= 0.25 and 1.0 - eq["saturated"] >= 0.10
    sat = P["saturated"]
    assert (sat["render"][sat["render"] == sat["target"]] == 1.0).all()
    assert np.abs(sat["render"].astype(np.float64) - sat["target"])[sat["render"] != sat["target"]].max() < 0.0101
    assert np.abs(P["blobs_near"]["render"].astype(np.float64) - P["blobs_near"]["target"]).max() < 0.12
    # the step stands on column 32, the target's on 33: one column differs
    col = ln.step_column(W)
    assert col == 32
    r, t = P["step_edge"]["render"], P["step_edge"]["target"]
    assert (r[:, :col] == 0).all() and (r[:, col:] == 1).all() and (t[:, :col + 1] == 0).all() and (t[:, col + 1:] == 1).all()
    assert abs(eq["step_edge"] - (1.0 - 1.0 / W)) < 1e-12
    # outside [0, 1] on both sides, mildly
    r = P["out_of_range"]["render"]
    assert 0.15 < out["out_of_range"] < 0.6 and -0.6 < r.min() < -0.2 and 1.2 < r.max() < 1.6
    assert all(out[n] == 0.0 for n in ALL if n != "out_of_range")
    # the zero band, in both images, across the seam at 32
    a, b = ln.ZERO_BAND
    assert a < 32 < b - 1
    r, t = P["zero_band"]["render"], P["zero_band"]["target"]
    assert (r[:, a:b] == 0).all() and (t[:, a:b] == 0).all() and (r[:, :a] != t[:, :a]).any() and (r[:, b:] != t[:, b:]).any()


def test_step_column_of_a_narrow_image():
    assert ln.step_column(9) == 4 and ln.step_column(32) == 16 and ln.step_column(33) == 32


@pytest.mark.parametrize("H,W,name", ln.CASES)
def test_cap_on_the_float32_oracles_own_cotangent_error(oracle32, oracle64, H, W, name):
    """err32 <= GRAD_RTOL max|cot64| wherever max|cot64| >= u: FACTOR err32 + GRAD_RTOL u is then at most 2.5e-3 of the largest
    cotangent.  Every (shape, pair) of the GPU test."""
    ref = ln.reference(oracle32, oracle64, name, H, W)
    c64 = ref["ref64"]["cot"]
    top, u = float(np.abs(c64).max()), ln.unit(c64.shape)
    err32 = float(np.abs(ref["ref32"]["cot"] - c64).max())
    if top >= u:
        assert err32 <= ln.GRAD_RTOL * top, (err32 / top, err32 / u)
    else:
        assert name in ln.EQUAL_PAIRS and top <= ZERO_COT * u and err32 <= ln.GRAD_RTOL * u, (top / u, err32 / u)
    # (the float32 oracle passes its own bars by construction)
    assert ln.misses(ln.bars(ref["ref32"], ref["ref64"], ref["ref32"])) == []


@pytest.mark.parametrize("H,W", ln.SHAPES_SSIM_OP)
def test_cap_on_the_float32_oracles_own_ssim_gradient_error(oracle32, oracle64, H, W):
    """The same cap for the op-level ssim / ssimVJP test (a random upstream, every pair): err32 <= GRAD_RTOL max|g64|.  The equal
    pairs' gradient is zero (ssim is at its maximum there; the float64 oracle leaves 1e-14 of the upstream), so their err32 --
    all the allowance they get -- is capped by the control's gradient instead: a thousandth of what noise has."""
    up = ln.ssim_upstream(H, W)
    g = {n: [ln.ssim_gradients(o, *ln.reference(oracle32, oracle64, n, H, W, images_only=True), up) for o in (oracle32, oracle64)]
         for n in ALL}
    control = min(np.abs(b).max() for b in g["noise"][1])
    for name in ALL:
        for a, b in zip(*g[name]):
            err32, top = np.abs(a - b).max(), np.abs(b).max()
            if name in ln.EQUAL_PAIRS:
                assert top <= 1e-12 * np.abs(up).max() and err32 <= ln.GRAD_RTOL * control, (name, top, err32)
            else:
                assert top >= control and err32 <= ln.GRAD_RTOL * top, (name, err32 / top)


def _rejections(oracle32, oracle64, mistake, H, W):
    """{pair: quantities beyond their bars} of one mistake at one shape, over the pairs it can act on."""
    rej = {}
    for name in ALL:
        ref = ln.reference(oracle32, oracle64, name, H, W)
        if not ln.mistake_can_act(mistake, H, W, ref["render"], ref["target"]):
            continue
        bad = ln.loss_statement(ref["render"], ref["target"], mistake=mistake)
        rej[name] = ln.misses(ln.bars(bad, ref["ref64"], ref["ref32"]))
    return rej


@pytest.mark.parametrize("H,W", SHAPES + [WHOLE_TILES])
@pytest.mark.parametrize("mistake", ln.MISTAKES)
def test_mistakes_are_rejected(oracle32, oracle64, mistake, H, W):
    rej = _rejections(oracle32, oracle64, mistake, H, W)
    print(mistake, (H, W), {n: v for n, v in rej.items()})
    if mistake == "ssim_mean_padded" and (H, W) == WHOLE_TILES:
        assert rej == {}                                    # cannot act: and is then no mistake at all
        ref = ln.reference(oracle32, oracle64, "noise", H, W)
        bad, good = (ln.loss_statement(ref["render"], ref["target"], mistake=m) for m in (mistake, None))
        assert bad["ssim"] == good["ssim"] and bad["loss"] == good["loss"] and np.array_equal(bad["cot"], good["cot"])
        return
    assert any(rej.values()), "no pair rejects it: the images are too tame"
    expect = REJECTED_BY[mistake]
    assert set(expect) <= set(rej)                           # it can act on each of them
    if mistake == "sign_zero_negative":
        expect = tuple(rej)                                  # and whatever else has equal pixels rejects it as well
    missing = [n for n in expect if not rej[n]]
    assert not missing, missing
