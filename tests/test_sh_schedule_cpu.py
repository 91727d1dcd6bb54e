"""The progressive SH degree without a device (gaussiansplattingmlx_amd/sh_schedule.py, include/gsplat.h gs_set_sh_degree,
DESIGN.md section 30): the schedule's table, the entry points' declaration, the trainer's refusals, and the yardstick the GPU
tests lean on -- the oracle's render_backward at degree d leaves exactly-zero features_rest gradients in the columns
>= Lact = 3 ((d + 1)^2 - 1).

Scene: tests/test_sparse_adam_cpu.py's scene(3000, 25) and its camera A.
"""
import importlib.util
import os
import re

import numpy as np
import pytest

from gaussiansplattingmlx_amd import sh_schedule as shs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = ("gs_set_sh_degree", "gs_get_sh_degree")
W, H = 160, 120


def _load(name):
    spec = importlib.util.spec_from_file_location("_shs_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------------- the schedule
def test_degree_at_table():
    s = shs.SHDegreeSchedule(start=0, every=1000)
    got = [s.degree_at(t, 4) for t in (0, 999, 1000, 3999, 4000, 29999)]      # on a degree-4 renderer
    assert got == [0, 0, 1, 3, 4, 4]
    s = shs.SHDegreeSchedule()                                                # the defaults are those
    assert (s.start, s.every, s.max_degree) == (0, 1000, None)
    s = shs.SHDegreeSchedule(start=2, every=1000)
    assert [s.degree_at(t, 4) for t in (0, 999, 1000, 2000, 5000)] == [2, 2, 3, 4, 4]
    s = shs.SHDegreeSchedule(start=0, every=1000, max_degree=3)
    assert [s.degree_at(t, 4) for t in (0, 2999, 3000, 4000, 29999)] == [0, 2, 3, 3, 3]
    assert [s.degree_at(t) for t in (3000, 29999)] == [3, 3]                  # (its own cap needs no renderer)
    assert shs.SHDegreeSchedule(max_degree=4).degree_at(29999, 2) == 2        # the renderer's maximum bounds max_degree
    s = shs.SHDegreeSchedule(every=3)
    assert [s.degree_at(t, 4) for t in range(10)] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3]
    assert [shs.active_columns(d) for d in range(5)] == [0, 9, 24, 45, 72]


@pytest.mark.parametrize("kw", [dict(every=0), dict(every=-1), dict(start=-1), dict(every=2.5), dict(start="0"), dict(every=True),
                                dict(max_degree=-1), dict(max_degree=1.5), dict(every=None)])
def test_schedule_refuses(kw):
    with pytest.raises(ValueError):
        shs.SHDegreeSchedule(**kw)


def test_degree_at_refuses_a_negative_iteration():
    with pytest.raises(ValueError):
        shs.SHDegreeSchedule().degree_at(-1, 4)


# ------------------------------------------------------------------------------------------------------------ entry points
def test_header_and_binding_declare_the_entries():
    src = open(os.path.join(ROOT, "include", "gsplat.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    from gaussiansplattingmlx_amd import _lib
    for e in ENTRIES:
        assert re.search(r"\bint " + e + r"\s*\(", plain), e
        assert e in _lib.exported_symbols()
        assert e in _lib._SIGS
    assert re.search(r"\bGS_TUNE_SH_BAND_SKIP\s*=\s*19\b", plain) and _lib.TUNE_SH_BAND_SKIP == 19
    assert re.search(r"#define GSPLAT_ABI_VERSION 6\b", src)


def test_abi_version_and_null_context():
    from gaussiansplattingmlx_amd import build, _lib
    import ctypes as C
    build.build()
    lib = _lib.load()
    assert lib.gs_abi_version() == 6
    d = C.c_int(7)
    assert lib.gs_set_sh_degree(None, 0) == 1
    assert lib.gs_get_sh_degree(None, C.byref(d)) == 1 and d.value == 7


# ------------------------------------------------------------------------------------------------------------- the trainer
@pytest.mark.parametrize("kw", [dict(process_group=object()), dict(dp_bootstrap=(b"", 0, 1)), dict(exchange_impl="native"),
                                dict(views_per_rank=2), dict(sh_schedule=1), dict(sh_schedule="yes"), dict(sh_schedule=True),
                                dict(sh_schedule=(0, 1000))])
def test_trainer_refuses(kw):
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    args = dict(sh_schedule=shs.SHDegreeSchedule())
    args.update(kw)
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, **args)        # refused before the model or the renderer is touched


def test_trainer_revalidates_the_schedule():
    from gaussiansplattingmlx_amd.trainer import GaussianTrainer
    s = shs.SHDegreeSchedule()
    s.every = 0
    with pytest.raises(ValueError):
        GaussianTrainer(None, None, sh_schedule=s)


# ------------------------------------------------------------------------------------- the oracle's inactive gradients are zero
@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_oracle_inactive_gradients_are_exact_zeros(oracle32, d):
    p, cams = _load("test_sparse_adam_cpu").scene(3000, 25)
    c = cams[0].as_dict()
    o = oracle32
    fw = o.render_forward(p, c, W, H, 16, 16, d)
    cot = (np.random.default_rng(3).standard_normal((W * H, 3)) / (W * H)).astype(np.float32)
    z = np.zeros(W * H, np.float32)
    g = o.render_backward(p, c, W, H, 16, 16, d, fw, cot, z, z)
    rest = np.asarray(g["features_rest"], np.float32).reshape(3000, 72)
    lact = shs.active_columns(d)
    assert not rest[:, lact:].view(np.uint32).any()        # +0.0, every bit
    if d > 0:
        live = np.abs(rest[:, :lact]).max(axis=0) > 0
        assert live.all()                                  # ... and every active column gets a gradient somewhere
    assert np.abs(np.asarray(g["features_dc"])).max() > 0
    # the forward at degree d does not read the inactive bands either
    q = dict(p)
    q["features_rest"] = p["features_rest"].copy()
    q["features_rest"].reshape(3000, 72)[:, lact:] = 7.0
    fw2 = o.render_forward(q, c, W, H, 16, 16, d)
    assert np.array_equal(np.asarray(fw2["color"]), np.asarray(fw["color"]))
