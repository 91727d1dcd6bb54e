"""The reference for a background colour, composed from the black oracle (gaussiansplattingmlx_amd/background.py's statements;
include/gsplat.h gs_set_background), and the scene the background tests share.

The oracle knows black and white only.  For a colour b:
    forward     colour_b = colour_black + (1 - alpha) b
    backward    the gradient for cotangents (g, cD, cA) under b is the black backward's for (g, cD, cA - g . b)
Scene: test_gpu_trajectory._scene(71, 3000, 160, 120, 0.03), camera 0.  Every oracle forward is computed once per
(precision, tile) and never written to.
"""
import importlib.util
import os

import numpy as np

from gaussiansplattingmlx_amd import background as bgm

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, N = 160, 120, 3000
B_IN = (0.9, 0.2, 0.55)             # inside the unit cube
B_OUT = (-0.5, 2.0, 0.0)            # outside it: the setter does not confine the colour
KEYS = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")

_cache = {}


def _load(name):
    spec = importlib.util.spec_from_file_location("_bgn_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def scene():
    if "scene" not in _cache:
        _cache["scene"] = _load("test_gpu_trajectory")._scene(71, N, W, H, 0.03)
    return _cache["scene"]


def forward(o, tile=(16, 16), white=False):
    """The oracle's forward of camera 0 over black (or white)."""
    key = ("fw", np.dtype(o.dtype).name, tuple(tile), bool(white))
    if key not in _cache:
        p, cams = scene()
        fw = o.render_forward(p, cams[0].as_dict(), W, H, tile[0], tile[1], 4, whiteBg=white)
        for k in ("color", "alpha", "depth"):
            fw[k].setflags(write=False)
        _cache[key] = fw
    return _cache[key]


def render_under(o, b, tile=(16, 16)):
    """(colour [H W, 3], alpha [H W], depth [H W]) of camera 0 over b."""
    fw = forward(o, tile)
    return bgm.with_background(fw["color"].reshape(-1, 3), fw["alpha"].reshape(-1), b), fw["alpha"], fw["depth"]


def backward_under(o, b, cot, cd, ca, tile=(16, 16), fw=None, p=None, cam=None, w=W, h=H):
    """The parameter gradients of camera 0 under b for cotangents (cot [.., 3], cd, ca; None = zeros): the black backward under
    the shifted alpha cotangent."""
    if fw is None:
        fw = forward(o, tile)
        p, cams = scene()
        cam = cams[0].as_dict()
    dt = o.dtype
    cot = np.asarray(cot, dt).reshape(-1, 3)
    z = np.zeros(w * h, dt)
    cd = z if cd is None else np.asarray(cd, dt).reshape(-1)
    ca = z if ca is None else np.asarray(ca, dt).reshape(-1)
    return o.render_backward(p, cam, w, h, tile[0], tile[1], 4, fw, cot, cd, bgm.shifted_cot_alpha(cot, ca, b))


def loss_under(o, p, cam, w, h, target, b, tile=(16, 16), lam=0.2):
    """(loss, the black forward, the colour cotangent) of the L1 + DSSIM loss of the render over b against target."""
    fw = o.render_forward(p, cam, w, h, tile[0], tile[1], 4)
    img = bgm.with_background(fw["color"].reshape(h, w, 3), fw["alpha"].reshape(h, w), b)
    loss, cot, _, _, _ = o.loss_forward_backward(img.astype(o.dtype), np.asarray(target, o.dtype), lam)
    return float(loss), fw, cot


def list_lengths(fw):
    r = np.asarray(fw["bin"].tileRanges).reshape(-1, 2).astype(np.int64)
    return r[:, 1] - r[:, 0]
