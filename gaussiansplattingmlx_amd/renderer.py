"""Host-side mirror of the reference's `GaussianRenderer` (Trainer/GaussianRenderer.swift) over the C ABI.

Same constructor, method names, argument meaning and result tuple as the reference class; every device
operation goes through libgsplat_hip.so (hand-written HIP).  torch is used only to own device memory and
the stream.  There is no CPU path: constructing a renderer without the library or a GPU raises, as the
reference's init preconditions do (GaussianRenderer.swift:721-733).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import _lib, loss_mask
from ._lib import GsplatError

TILE_SIZE_H_W = namedtuple("TILE_SIZE_H_W", ["w", "h"])
RenderResult = namedtuple("RenderResult", ["render", "depth", "alpha", "visiility_filter", "radii"])


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _f32(t, device):
    if isinstance(t, torch.Tensor):
        return t.to(device=device, dtype=torch.float32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32), device=device)


class CutPolicy:
    """When does a training view bin under depth cuts (gs_set_view_hints)?  The cuts cost a fixed ~40 us per forward
    (second expansion pass, the host's wait for the forward, an occasional repeated forward) and save ~13 us per
    million pairs they leave out (MI355X, 300 k Gaussians at 800x800: 4.4 M left out = break-even; round 5: 7.3 M left out on
    the same scene at 200 x 200 tiles = +1.5 %, hence the default of 6 M).  So: never on
    a forward while the view's cuts are empty -- they are written by the backward's preparation (loss or backward of
    a forward of the view), so a view that has only been rendered has none -- and a view whose cuts left out fewer than
    min_dropped pairs sits out the next probe_interval forwards, then is tried again."""

    def __init__(self, min_dropped: int = 6_000_000, probe_interval: int = 64):
        self.min_dropped, self.probe_interval = min_dropped, probe_interval
        self.sit_out = 0            # forwards still to run without cuts
        self.last_dropped = 0       # pairs the last cut forward left out
        self.since_empty = 0        # backward preparations since the view's cuts were last empty (0: they are empty now)

    def begin(self, allowed: bool) -> bool:
        """Called once per forward of the view; True = run this one under cuts."""
        use = allowed and self.sit_out == 0 and self.since_empty >= 1
        if allowed and self.sit_out > 0:
            self.sit_out -= 1
        return use

    def renewed(self):
        """The backward's preparation of a forward of this view has been queued: the view's cuts exist from now on."""
        self.since_empty += 1

    def report(self, missed: bool, kept: int, full: int):
        """After a forward under cuts: kept / full pairs (gs_cut_stats)."""
        self.last_dropped = max(int(full) - int(kept), 0)
        if not missed and full > 0 and self.last_dropped < self.min_dropped:
            self.sit_out = self.probe_interval

    def cuts_cleared(self):
        self.since_empty = 0


class GaussianRenderer:
    def __init__(self, active_sh_degree: int, W: int, H: int, TILE_SIZE=TILE_SIZE_H_W(16, 16),
                 whiteBackground: bool = False, useScreenSpaceCustomOp: bool = True, device: int = 0,
                 antialiased: bool = False):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("GaussianRenderer needs a GPU: the HIP path has no CPU fallback")
        self.active_sh_degree, self.W, self.H = int(active_sh_degree), int(W), int(H)
        self.TILE_SIZE = TILE_SIZE_H_W(*TILE_SIZE)
        self.whiteBackground = bool(whiteBackground)
        self.useScreenSpaceCustomOp = useScreenSpaceCustomOp
        self.device = torch.device("cuda", device)
        self.profiler = None          # an IntervalProfiler the trainer sets per profiled iteration (GaussianRenderer.swift:66-68)
        torch.cuda.set_device(self.device)
        ctx = C.c_void_p()
        rc = self.lib.gs_ctx_create(device, self.W, self.H, self.TILE_SIZE.w, self.TILE_SIZE.h,
                                    self.active_sh_degree, int(self.whiteBackground), C.byref(ctx))
        if rc != _lib.GS_OK:
            raise GsplatError(rc, "gs_ctx_create failed")
        self.ctx = ctx
        self._check(self.lib.gs_ctx_set_stream(self.ctx, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        win = np.zeros(121, np.float32)
        self.lib.gs_ssim_window(11, C.c_float(1.5), win.ctypes.data_as(C.c_void_p))
        self.ssimWindow = torch.as_tensor(win, device=self.device)
        self._saved = {}
        self.reserved = None
        self._grad_norm_accum = None
        self._work_hints = {}
        self.depthCuts = True          # False: view hints order the forward's work but never cut the binning
        self._cut_policy = {}          # viewKey -> CutPolicy
        self._cut_view = None
        self._hinted_view = None
        self.cutMinDropped = 6_000_000      # (c3 at 16 x 16 tiles leaves out 4 - 5 M: break-even, off; at the app's 200 x 200 tiles 7.3 M: +1.5 %; c5 80 M)
        self.cutProbeInterval = 64
        # 16 x 16 tiles, or a tile size that is not a multiple of 16 (the library then works on block lists: gs_ctx.h)
        self._hints_ok = (self.TILE_SIZE.w, self.TILE_SIZE.h) == (16, 16) or \
            ((self.TILE_SIZE.w % 16 != 0 or self.TILE_SIZE.h % 16 != 0) and os.environ.get("GSPLAT_BLOCK_LISTS", "1") != "0")
        self.targetStatsCache = True   # lossForwardBackward(targetKey=...) keeps the target's SSIM statistics per key
        self._target_cache = OrderedDict()
        self.targetStatsCacheBytes = 8 << 30      # cap of the per-view caches together (6 H W floats each); LRU beyond it
        self._antialiased = False
        self._camera_model = "pinhole"
        self._sh_degree = self.active_sh_degree      # (the library's default: the maximum)
        self._absgrad = False
        self._sparse_adam = False
        self._background = None
        self._exposure = (None, None)  # setExposure's tensors while the library holds their addresses
        self._bilateral = (None, None)  # setBilateralGrid's, likewise
        self._loss_mask = None         # setLossMask's uint8 device tensor, likewise
        self._distortion_armed = None  # armDistortion's (cot, totals), likewise, until the next arming
        if antialiased:
            self.setAntialiased(True)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.gs_set_block_work_buffer(self.ctx, None)
            self.lib.gs_set_loss_target_cache(self.ctx, None, 0)
            self.lib.gs_set_loss_mask(self.ctx, None)
            self.lib.gs_set_grad_norm_accum(self.ctx, None)
            self.lib.gs_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing ---------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != _lib.GS_OK:
            raise GsplatError(rc, self.lib.gs_last_error(self.ctx).decode())

    def _t(self, t):
        return _f32(t, self.device)

    def _measure(self, name, body):
        """Runs body inside the profiler's section `name` when the trainer has set one (GaussianRenderer.swift:157-172,
        579-600), plainly otherwise."""
        return self.profiler.measure(name, body) if self.profiler is not None else body()

    def _empty(self, *shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def reserve(self, max_gaussians: int, max_pairs: int):
        self._check(self.lib.gs_ctx_reserve(self.ctx, int(max_gaussians), int(max_pairs)))
        self.reserved = (int(max_gaussians), int(max_pairs))

    def sync(self):
        self._check(self.lib.gs_sync(self.ctx))

    _TUNING = dict(fwd_waves_per_simd=_lib.TUNE_FWD_WAVES_PER_SIMD, bwd_waves_per_cu=_lib.TUNE_BWD_WAVES_PER_CU,
                   fwd_quadrants=_lib.TUNE_FWD_QUADRANTS, op_fwd_ppl=_lib.TUNE_OP_FWD_PPL,
                   op_bwd_ppl=_lib.TUNE_OP_BWD_PPL, fwd_trace_buffer=_lib.TUNE_FWD_TRACE_BUFFER,
                   depth_gradient=_lib.TUNE_DEPTH_GRADIENT, wide_tile_sort=_lib.TUNE_WIDE_TILE_SORT,
                   host_overflow_errors=_lib.TUNE_HOST_OVERFLOW_ERRORS, splitter_depth_sort=_lib.TUNE_SPLITTER_DEPTH_SORT,
                   colour_riders=_lib.TUNE_COLOUR_RIDERS, fwd_queues=_lib.TUNE_FWD_QUEUES, fwd_four_waves=_lib.TUNE_FWD_FOUR_WAVES,
                   fwd_fold_test_scale=_lib.TUNE_FWD_FOLD_TEST_SCALE, poison_checkpoints=_lib.TUNE_POISON_CHECKPOINTS,
                   render_only=_lib.TUNE_RENDER_ONLY, fwd_pair=_lib.TUNE_FWD_PAIR, fwd_slow_slot=_lib.TUNE_FWD_SLOW_SLOT,
                   trim_rects=_lib.TUNE_TRIM_RECTS, sh_band_skip=_lib.TUNE_SH_BAND_SKIP)
    _TUNING_DEFAULTS = dict(fwd_waves_per_simd=4, bwd_waves_per_cu=16, fwd_quadrants=1, op_fwd_ppl=1, op_bwd_ppl=1,
                            fwd_trace_buffer=0, depth_gradient=1, wide_tile_sort=1, host_overflow_errors=1, splitter_depth_sort=1,
                            colour_riders=1, fwd_queues=8, fwd_four_waves=-1, fwd_fold_test_scale=1000, poison_checkpoints=0, render_only=0, fwd_pair=-1, fwd_slow_slot=3, trim_rects=2,
                            sh_band_skip=1)

    def setTuning(self, **knobs):
        """Launch tuning of THIS renderer's context (gs_ctx_set_tuning); results never depend on it (fwd_four_waves: within
        the parity bars, not to the bit -- sums composed across list chunks instead of accumulated)."""
        for k, v in knobs.items():
            self._check(self.lib.gs_ctx_set_tuning(self.ctx, self._TUNING[k], int(v)))
            self._tuning_now = {**getattr(self, "_tuning_now", {}), k: int(v)}

    def getTuning(self, knob: str) -> int:
        """The value this renderer last set for a knob (the library's default if it never did)."""
        return getattr(self, "_tuning_now", {}).get(knob, self._TUNING_DEFAULTS[knob])

    def colourRidersActive(self, N: int, K: int = 25) -> bool:
        """Do the fused forwards of N Gaussians (from this context's second one on) compute their SH colours as rider workgroups of
        the binning kernels (csrc/projection.hip: K = 25, GS_TUNE_COLOUR_RIDERS = 1 and a depth sort that takes the splitter
        buckets -- 16385 .. 655 360 records by default, binning.hip ss_fits)?  bench.py: the projection stage's time then holds
        the geometry half only."""
        if K != 25 or self.getTuning("colour_riders") != 1 or ((self.TILE_SIZE.w % 16 or self.TILE_SIZE.h % 16) and not self.blockLists):
            return False
        return bool(self.getTuning("splitter_depth_sort")) and 16384 < N <= 160 * 4096

    def stats(self):
        s = (C.c_uint32 * 8)()
        self._check(self.lib.gs_last_stats(self.ctx, s))
        return dict(N_visible=s[0], M=s[1], max_tile_list=s[2], overflow=s[5], capN=s[6], capM=s[7])

    @staticmethod
    def _camera(viewMatrix, projMatrix, cameraCenter, fovX, fovY, focalX, focalY):
        g = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
        return _lib.make_camera(g(viewMatrix), g(projMatrix), g(cameraCenter), float(g(fovX)), float(g(fovY)),
                                float(g(focalX)), float(g(focalY)))

    # -- activations (GaussianRenderer.swift:936-963) ------------------------------------------------
    def get_scales_from(self, scales):
        return torch.exp(scales)

    def get_rotation_from(self, rotation):
        return rotation / (torch.sqrt(torch.sum(rotation * rotation, dim=1, keepdim=True)) + 1e-8)

    def get_xyz_from(self, xyz):
        return xyz

    def get_features_from(self, features_dc, features_rest):
        return torch.cat([features_dc, features_rest], dim=1)

    def get_opacity_from(self, opacity):
        return torch.sigmoid(opacity)

    # -- projection custom function (GaussianRenderer.swift:494-603) -----------------------------------
    def projectionScreenFused(self, scales, rotations, means3d, shs, cam):
        scales, rotations, means3d, shs = map(self._t, (scales, rotations, means3d, shs))
        N, K = means3d.shape[0], shs.shape[1]
        out = dict(means2d=self._empty(N, 2), depths=self._empty(N), color=self._empty(N, 3),
                   cov2d=self._empty(N, 2, 2), conic=self._empty(N, 2, 2), radii=self._empty(N),
                   rectMin=self._empty(N, 2), rectMax=self._empty(N, 2))
        self._check(self.lib.gs_projection_forward(
            self.ctx, N, K, _p(scales), _p(rotations), _p(means3d), _p(shs), C.byref(cam), _p(out["means2d"]),
            _p(out["depths"]), _p(out["color"]), _p(out["cov2d"]), _p(out["conic"]), _p(out["radii"]),
            _p(out["rectMin"]), _p(out["rectMax"])))
        return out

    def projectionScreenFusedVJP(self, scales, rotations, means3d, shs, cam, cotMeans2d, cotDepths, cotColor,
                                 cotCov2d, cotConic):
        scales, rotations, means3d, shs = map(self._t, (scales, rotations, means3d, shs))
        cotMeans2d, cotDepths, cotColor, cotCov2d, cotConic = map(self._t, (cotMeans2d, cotDepths, cotColor,
                                                                            cotCov2d, cotConic))
        N, K = means3d.shape[0], shs.shape[1]
        out = dict(gradScales=self._empty(N, 3), gradRot=self._empty(N, 4), gradMeans3d=self._empty(N, 3),
                   gradShs=self._empty(N, K, 3), gradCamCenterPoint=self._empty(N, 3))
        self._measure("bwd.projectionScreenFused", lambda: self._check(self.lib.gs_projection_backward(
            self.ctx, N, K, _p(scales), _p(rotations), _p(means3d), _p(shs), C.byref(cam), _p(cotDepths),
            _p(cotMeans2d), _p(cotCov2d), _p(cotColor), _p(cotConic), _p(out["gradScales"]), _p(out["gradRot"]),
            _p(out["gradMeans3d"]), _p(out["gradShs"]), _p(out["gradCamCenterPoint"]))))
        out["gradCameraCenter"] = out["gradCamCenterPoint"].sum(dim=0, keepdim=True)   # :683-684
        return out

    # -- tile binning (GaussianRenderer.swift:333-490) -----------------------------------------------------
    def buildGlobalTileSliceInfo(self, rect, radii, depths, want_dense: bool = False, tileCuts=None):
        """tileCuts: optional u32 [T] per-tile depth cuts (gs_tile_bin_cut: 0 = none, else 0xFFFFFFFF - the largest depth
        key still binned in that tile); the lists are then prefixes of the reference's."""
        rmin, rmax, radii, depths = self._t(rect[0]), self._t(rect[1]), self._t(radii), self._t(depths)
        N = radii.shape[0]
        if tileCuts is None:
            self._check(self.lib.gs_tile_bin(self.ctx, N, _p(rmin), _p(rmax), _p(radii), _p(depths)))
        else:
            cuts = torch.as_tensor(np.ascontiguousarray(tileCuts, dtype=np.uint32).view(np.int32), device=self.device)
            self._check(self.lib.gs_tile_bin_cut(self.ctx, N, _p(rmin), _p(rmax), _p(radii), _p(depths), _p(cuts)))
        M, B = C.c_uint32(), C.c_uint32()
        self._check(self.lib.gs_tile_bin_info(self.ctx, C.byref(M), C.byref(B)))
        T = ((self.W + self.TILE_SIZE.w - 1) // self.TILE_SIZE.w) * ((self.H + self.TILE_SIZE.h - 1) // self.TILE_SIZE.h)
        info = dict(M=M.value, maxTilePairs=B.value, numTiles=T)
        info["sortedGaussIdx"] = self._empty(M.value, dtype=torch.int32)
        info["tileRanges"] = self._empty(T, 2, dtype=torch.int32)
        info["tileCounts"] = self._empty(T, dtype=torch.int32)
        self._check(self.lib.gs_tile_bin_export(self.ctx, _p(info["sortedGaussIdx"]), _p(info["tileRanges"]),
                                                _p(info["tileCounts"])))
        if want_dense:
            dense = torch.zeros((T, B.value), dtype=torch.int32, device=self.device)
            self._check(self.lib.gs_build_packed_tile_indices(self.ctx, B.value, _p(dense)))
            info["packedTileIndices"] = dense
        return info

    def buildPackedGaussians(self, means2d, conic, color, opacity, depths):
        means2d, conic, color, opacity, depths = map(self._t, (means2d, conic, color, opacity, depths))
        N = means2d.shape[0]
        packed = self._empty(N, 11)
        self._check(self.lib.gs_pack_gaussians(self.ctx, N, _p(means2d), _p(conic), _p(color), _p(opacity),
                                               _p(depths), _p(packed)))
        return packed

    # -- tile composite custom function (GaussianRenderer.swift:101-244) -----------------------------------
    def globalTileComposite(self, packedGaussians):
        packed = self._t(packedGaussians)
        P = self.W * self.H
        color, depth, alpha = self._empty(P, 3), self._empty(P), self._empty(P)
        last = self._empty(P, dtype=torch.int32)
        self._check(self.lib.gs_blend_forward(self.ctx, packed.shape[0], _p(packed), _p(color), _p(depth), _p(alpha),
                                              _p(last)))
        self._saved = dict(packed=packed, color=color, depth=depth, alpha=alpha, last=last)
        return color, depth, alpha

    def globalTileCompositeVJP(self, cotColor, cotDepth=None, cotAlpha=None, saved=None):
        s = saved or self._saved
        packed = s["packed"]
        cotColor = self._t(cotColor)
        cotDepth = None if cotDepth is None else self._t(cotDepth)
        cotAlpha = None if cotAlpha is None else self._t(cotAlpha)
        grad = self._empty(packed.shape[0], 11)
        self._measure("bwd.globalTileComposite", lambda: self._check(self.lib.gs_blend_backward(
            self.ctx, packed.shape[0], _p(packed), _p(cotColor), _p(cotDepth), _p(cotAlpha), _p(s["color"]),
            _p(s["depth"]), _p(s["alpha"]), _p(s["last"]), _p(grad))))
        return grad

    # -- per-Gaussian blend weight scores (include/gsplat.h gs_blend_contrib) -------------
    def _contrib_out(self, who, N, maxW, sumW):
        if maxW is None and sumW is None:
            raise ValueError(f"{who}: one of maxW, sumW at least")
        for name, t in (("maxW", maxW), ("sumW", sumW)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
                                      and t.is_contiguous() and t.numel() == N):
                raise ValueError(f"{who}: {name} must be a contiguous float32 device tensor of {N} elements")

    def blendContrib(self, packedGaussians, maxW=None, sumW=None):
        """The blend weight scores of the view whose lists the last buildGlobalTileSliceInfo built: per Gaussian the maximum
        and the sum over the pixels of w = T alpha.  ACCUMULATES into maxW / sumW (float32 device tensors [N], either may be
        None): maxW becomes max(old, this view), sumW gets this view added."""
        packed = self._t(packedGaussians)
        N = int(packed.shape[0])
        self._contrib_out("blendContrib", N, maxW, sumW)
        self._check(self.lib.gs_blend_contrib(self.ctx, N, _p(packed), _p(maxW), _p(sumW)))
        return maxW, sumW

    def renderContrib(self, maxW=None, sumW=None):
        """blendContrib for the view of the last renderForward / renderChecked, on that forward's own records and lists (its
        anti-aliased opacity, 3-D filter and pose correction included).  Consumes nothing: a renderBackward may follow."""
        if getattr(self, "_fused", None) is None:
            raise GsplatError(5, "renderContrib: no renderForward on this renderer")
        N = int(self._fused["params"]["xyz"].shape[0])
        self._contrib_out("renderContrib", N, maxW, sumW)
        self._check(self.lib.gs_render_contrib(self.ctx, _p(maxW), _p(sumW)))
        return maxW, sumW

    def contributionScores(self, params: dict, cameras, viewKeys=None):
        """(max_w, sum_w) [N] over `cameras`: every camera is rendered with renderChecked (no depth image; a forward that
        missed under depth cuts is repeated) and scored with renderContrib.  viewKeys: the cameras' view keys, or None."""
        cameras = list(cameras)
        if viewKeys is not None and len(viewKeys) != len(cameras):
            raise ValueError("contributionScores: one view key per camera")
        N = int(params["xyz"].shape[0])
        maxW, sumW = self._empty(N).zero_(), self._empty(N).zero_()
        for i, cam in enumerate(cameras):
            self.renderChecked(params, cam, viewKey=None if viewKeys is None else viewKeys[i], wantDepth=False)
            self.renderContrib(maxW, sumW)
        return maxW, sumW

    def contribActions(self, score, threshold: float):
        """(actions, counts) of classifyGaussians' kind from a score: prune (3, 0) where score < threshold, else keep (0, 1)."""
        score = self._t(score)
        N = int(score.shape[0])
        actions, counts = self._empty(N, dtype=torch.int32), self._empty(N, dtype=torch.int32)
        self._check(self.lib.gs_contrib_actions(self.ctx, N, _p(score), C.c_float(threshold), _p(actions), _p(counts)))
        return actions, counts

    # -- N-channel feature rendering (include/gsplat.h gs_blend_features) ---------------------
    def _feature_arg(self, who, name, t, rows, C):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                and t.numel() == rows * C):
            raise ValueError(f"{who}: {name} must be a contiguous float32 device tensor of {rows} x {C} elements")

    def _feature_channels(self, who, t, rows):
        """C of a [rows, C] (or [H, W, C]) tensor: its last dimension."""
        if not isinstance(t, torch.Tensor) or t.dim() < 2 or rows <= 0 or t.numel() % rows:
            raise ValueError(f"{who}: a float32 device tensor with the channels as its last dimension")
        C_ = int(t.shape[-1])
        if not 1 <= C_ <= _lib.MAX_FEATURE_CHANNELS:
            raise ValueError(f"{who}: 1 <= C <= {_lib.MAX_FEATURE_CHANNELS}, got {C_}")
        return C_

    def _features_forward(self, who, N, features, out, call):
        C_ = self._feature_channels(who, features, N)
        self._feature_arg(who, "features", features, N, C_)
        if out is None:
            out = self._empty(self.H, self.W, C_)
        self._feature_arg(who, "out", out, self.H * self.W, C_)
        self._check(call(C_, _p(features), _p(out)))
        return out

    def _features_backward(self, who, N, cot, grad, call):
        C_ = self._feature_channels(who, cot, self.H * self.W)
        self._feature_arg(who, "cot", cot, self.H * self.W, C_)
        if grad is None:
            grad = torch.zeros((N, C_), dtype=torch.float32, device=self.device)
        self._feature_arg(who, "grad", grad, N, C_)
        self._check(call(C_, _p(cot), _p(grad)))
        return grad

    def blendFeatures(self, packedGaussians, features, out=None):
        """The feature image [H, W, C] of the view whose lists the last buildGlobalTileSliceInfo built: out[p] = sum over the
        entries of p's list of w(p, g) features[g] with blendContrib's weights.  features: float32 device tensor [N, C],
        1 <= C <= 256.  Every pixel of out is written (out=None allocates); the same bits on every run."""
        packed = self._t(packedGaussians)
        N = int(packed.shape[0])
        return self._features_forward("blendFeatures", N, features, out,
                                      lambda C_, f, o: self.lib.gs_blend_features(self.ctx, N, C_, _p(packed), f, o))

    def blendFeaturesVJP(self, packedGaussians, cot, grad=None):
        """The gradient of blendFeatures with respect to the features for the cotangent image cot [H, W, C]:
        grad[g] += sum over the pixels of w(p, g) cot[p].  ACCUMULATES into grad [N, C] (grad=None: zeros are allocated)."""
        packed = self._t(packedGaussians)
        N = int(packed.shape[0])
        return self._features_backward("blendFeaturesVJP", N, cot, grad,
                                       lambda C_, ct, g: self.lib.gs_blend_features_backward(self.ctx, N, C_, _p(packed), ct, g))

    def renderFeatures(self, features, out=None):
        """blendFeatures for the view of the last renderForward / renderChecked, on that forward's own records and lists (its
        anti-aliased opacity, 3-D filter and pose correction included).  Consumes nothing: a renderBackward may follow."""
        if getattr(self, "_fused", None) is None:
            raise GsplatError(5, "renderFeatures: no renderForward on this renderer")
        N = int(self._fused["params"]["xyz"].shape[0])
        return self._features_forward("renderFeatures", N, features, out,
                                      lambda C_, f, o: self.lib.gs_render_features(self.ctx, C_, f, o))

    def renderFeaturesVJP(self, cot, grad=None):
        """blendFeaturesVJP for the view of the last renderForward / renderChecked.  ACCUMULATES into grad [N, C]."""
        if getattr(self, "_fused", None) is None:
            raise GsplatError(5, "renderFeaturesVJP: no renderForward on this renderer")
        N = int(self._fused["params"]["xyz"].shape[0])
        return self._features_backward("renderFeaturesVJP", N, cot, grad,
                                       lambda C_, ct, g: self.lib.gs_render_features_backward(self.ctx, C_, ct, g))

    # -- depth distortion loss (include/gsplat.h gs_blend_distortion; distortion.py) ------------
    @staticmethod
    def distortionParams(map="ndc", near: float = 0.2, far: float = 1000.0):
        """gs_distortion_params: the depth map by name (distortion.MAPS) and the "ndc" map's planes."""
        from .distortion import MAPS
        if map not in MAPS:
            raise ValueError(f"distortionParams: unknown map {map!r} (one of {', '.join(MAPS)})")
        return _lib.gs_distortion_params(MAPS.index(map), float(near), float(far))

    def _distortion_params(self, params):
        if params is None:
            return self.distortionParams()
        return params if isinstance(params, _lib.gs_distortion_params) else self.distortionParams(**params)

    def _image_arg(self, who, name, t, per_pixel=1):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                and t.numel() == self.H * self.W * per_pixel):
            raise ValueError(f"{who}: {name} must be a contiguous float32 device tensor of {self.H} x {self.W}"
                             + (f" x {per_pixel}" if per_pixel > 1 else "") + " elements")

    def _distortion_forward(self, who, params, out, totals, call):
        out = self._empty(self.H, self.W) if out is None else out
        totals = self._empty(self.H, self.W, 3) if totals is None else totals
        self._image_arg(who, "out", out)
        self._image_arg(who, "totals", totals, 3)
        p = self._distortion_params(params)
        self._check(call(C.byref(p), _p(out), _p(totals)))
        return out, totals

    def _distortion_backward(self, who, N, params, cot, totals, rows, call):
        self._image_arg(who, "cot", cot)
        self._image_arg(who, "totals", totals, 3)
        if rows is None:
            rows = torch.zeros((N, 16), dtype=torch.float32, device=self.device)
        if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous()
                and tuple(rows.shape) == (N, 16)):
            raise ValueError(f"{who}: rows must be a contiguous float32 device tensor [{N}, 16]")
        p = self._distortion_params(params)
        self._check(call(C.byref(p), _p(cot), _p(totals), _p(rows)))
        return rows

    def blendDistortion(self, packedGaussians, params=None, out=None, totals=None):
        """(D [H, W], totals [H, W, 3]) of the view whose lists the last buildGlobalTileSliceInfo built: the depth distortion
        D = sum_{i<j} w_i w_j (m_i - m_j)^2 of every pixel (2DGS eq. 13, gsplat's distloss) with blendContrib's weights, and
        the pixel's (A, mu, S), the backward's input.  params: distortionParams(...), a dict of its arguments, or None for its
        defaults.  Every pixel of both is written (None allocates); the same bits on every run."""
        packed = self._t(packedGaussians)
        N = int(packed.shape[0])
        return self._distortion_forward("blendDistortion", params, out, totals,
                                        lambda p, o, t: self.lib.gs_blend_distortion(self.ctx, N, _p(packed), p, o, t))

    def blendDistortionVJP(self, packedGaussians, cot, totals, params=None, rows=None):
        """The gradient of sum_p cot[p] D[p] with respect to the packed records, as rows [N, 16] in the column order of the blend
        backward's accumulator (dmx dmy dc00 dc01 | dc10 dc11 dr dg | db dop ddepth): columns 0 .. 5, 9 and 10 ACCUMULATE
        (rows=None: zeros are allocated), the others are not touched.  totals: what blendDistortion returned."""
        packed = self._t(packedGaussians)
        N = int(packed.shape[0])
        return self._distortion_backward("blendDistortionVJP", N, params, cot, totals, rows,
                                         lambda p, c, t, r: self.lib.gs_blend_distortion_backward(self.ctx, N, _p(packed), p, c, t, r))

    def renderDistortion(self, params=None, out=None, totals=None):
        """blendDistortion for the view of the last renderForward / renderChecked, on that forward's own records and lists (its
        anti-aliased opacity, 3-D filter and pose correction included).  Consumes nothing: a renderBackward may follow."""
        if getattr(self, "_fused", None) is None:
            raise GsplatError(5, "renderDistortion: no renderForward on this renderer")
        return self._distortion_forward("renderDistortion", params, out, totals,
                                        lambda p, o, t: self.lib.gs_render_distortion(self.ctx, p, o, t))

    def renderDistortionVJP(self, cot, totals, params=None, rows=None):
        """blendDistortionVJP for the view of the last renderForward / renderChecked.  ACCUMULATES into rows [N, 16]."""
        if getattr(self, "_fused", None) is None:
            raise GsplatError(5, "renderDistortionVJP: no renderForward on this renderer")
        N = int(self._fused["params"]["xyz"].shape[0])
        return self._distortion_backward("renderDistortionVJP", N, params, cot, totals, rows,
                                         lambda p, c, t, r: self.lib.gs_render_distortion_backward(self.ctx, p, c, t, r))

    def distortionLoss(self, distort, weight: float, mask=None, loss=None, cot=None):
        """gs_distortion_loss on a distortion image [H, W]: returns (loss, cot) with loss[0] += weight (1 / (H W)) sum_p v_p D_p
        and cot [H, W] = weight v_p / (H W), v = mask / 255 of an optional uint8 device tensor [H, W] (None: 1).  loss: the
        float tensor a lossForwardBackward has written (zeros of one element without it); cot=None allocates."""
        self._image_arg("distortionLoss", "distort", distort)
        if mask is not None and not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype == torch.uint8
                                     and mask.is_contiguous() and mask.numel() == self.H * self.W):
            raise ValueError(f"distortionLoss: mask is a contiguous uint8 device tensor [{self.H}, {self.W}], or None")
        if loss is None:
            loss = torch.zeros(1, device=self.device)
        if not (isinstance(loss, torch.Tensor) and loss.is_cuda and loss.dtype == torch.float32 and loss.numel() >= 1):
            raise ValueError("distortionLoss: loss is a float32 device tensor of at least one element")
        cot = self._empty(self.H, self.W) if cot is None else cot
        self._image_arg("distortionLoss", "cot", cot)
        self._check(self.lib.gs_distortion_loss(self.ctx, C.c_float(weight), self.H * self.W, _p(distort), _p(mask), _p(loss),
                                                _p(cot)))
        return loss, cot

    def armDistortion(self, cot=None, totals=None, params=None):
        """Arms the distortion term for the current forward: the next renderBackward / renderBackwardAdam of it adds
        renderDistortionVJP(cot, totals) to the library's own accumulator rows, behind the blend backward and in front of the
        ADC statistic and the projection backward.  cot and totals None: disarms (a new renderForward disarms too).  The two
        tensors are held until then."""
        if cot is None and totals is None:
            self._check(self.lib.gs_arm_distortion(self.ctx, None, None, None))
            self._distortion_armed = None
            return
        self._image_arg("armDistortion", "cot", cot)
        self._image_arg("armDistortion", "totals", totals, 3)
        p = self._distortion_params(params)
        self._check(self.lib.gs_arm_distortion(self.ctx, C.byref(p), _p(cot), _p(totals)))
        self._distortion_armed = (cot, totals)      # (the library holds their addresses)

    # -- render / forward (GaussianRenderer.swift:736-934) ---------------------------------------------------
    def render(self, imageWidth, imageHeight, means2d, cov2d, color, opacity, depths, radii, conic, rect,
               inputIsDepthSorted: bool = False):
        if imageWidth != self.W or imageHeight != self.H:
            raise GsplatError(2, f"Renderer image size mismatch: expected ({self.W}, {self.H}), got "
                                 f"({imageWidth}, {imageHeight})")
        packed = self.buildPackedGaussians(means2d, conic, color, opacity, depths)
        radii_t, depths_t = self._t(radii), self._t(depths)
        N = radii_t.shape[0]
        self._check(self.lib.gs_tile_bin(self.ctx, N, _p(self._t(rect[0])), _p(self._t(rect[1])), _p(radii_t),
                                         _p(depths_t)))
        c, d, a = self.globalTileComposite(packed)
        return RenderResult(c.view(self.H, self.W, 3), d.view(self.H, self.W, 1), a.view(self.H, self.W, 1),
                            radii_t > 0, radii_t)

    def forwardWithCameraParams(self, viewMatrix, projMatrix, cameraCenter, fovX, fovY, focalX, focalY, imageWidth,
                                imageHeight, means3d, shs, opacity, scales, rotations):
        cam = self._camera(viewMatrix, projMatrix, cameraCenter, fovX, fovY, focalX, focalY)
        scales, rotations, means3d, shs = map(self._t, (scales, rotations, means3d, shs))
        o = self.projectionScreenFused(scales, rotations, means3d, shs, cam)
        res = self.render(imageWidth, imageHeight, o["means2d"], o["cov2d"], o["color"], opacity, o["depths"],
                          o["radii"], o["conic"], (o["rectMin"], o["rectMax"]))
        # what the VJP chain needs (the reference keeps it in the closures of its two custom functions)
        self._chain = dict(cam=cam, scales=scales, rotations=rotations, means3d=means3d, shs=shs, blend=self._saved)
        return res

    def forwardWithCameraParamsVJP(self, cotRender, cotDepth=None, cotAlpha=None):
        """The VJP MLX composes for forwardWithCameraParams (GaussianTrainer.swift:719-722 over
        GaussianRenderer.swift:149-185, 85-99, 605-701): blend VJP -> split of gradPacked along buildPackedGaussians'
        columns -> projection VJP.  Returns the gradients w.r.t. the ACTIVATED inputs means3d, shs, opacity, scales,
        rotations (the activation VJPs are the host framework's, as in the reference) plus gradPacked itself."""
        ch = self._chain
        gp = self.globalTileCompositeVJP(cotRender, cotDepth, cotAlpha, saved=ch["blend"])
        N = gp.shape[0]
        # packed columns (GaussianRenderer.swift:45-51): means2d 0:2, conic 2:6, colour 6:9, opacity 9, depth 10
        pb = self.projectionScreenFusedVJP(ch["scales"], ch["rotations"], ch["means3d"], ch["shs"], ch["cam"],
                                           gp[:, 0:2], gp[:, 10], gp[:, 6:9], torch.zeros(N, 4, device=self.device),
                                           gp[:, 2:6])
        return dict(means3d=pb["gradMeans3d"], shs=pb["gradShs"], opacity=gp[:, 9].contiguous(), scales=pb["gradScales"],
                    rotations=pb["gradRot"], gradPacked=gp, gradCameraCenter=pb["gradCameraCenter"])

    def forward(self, camera, means3d, shs, opacity, scales, rotations):
        return self.forwardWithCameraParams(camera.worldViewTransform, camera.projectionMatrix, camera.cameraCenter,
                                            camera.FoVx, camera.FoVy, camera.focalX, camera.focalY,
                                            camera.imageWidth, camera.imageHeight, means3d, shs, opacity, scales,
                                            rotations)

    # -- fused raw-parameter path (the trainer's lossFn, GaussianTrainer.swift:652-686) ------------------------
    def renderForward(self, params: dict, camera, want_radii: bool = False, viewKey=None, depthCuts: bool = True,
                      wantDepth: bool = True):
        """params: raw tensors xyz, features_dc, features_rest, scales, rotation, opacity (device f32).
        wantDepth=False: no depth image (RenderResult.depth is None; a train step without a depth term reads none, and
        the blend then carries no depth sum); the backward of such a forward takes no depth cotangent.
        viewKey: any hashable naming the camera (e.g. the training view index).  When given, the per-block sweep
        lengths this forward measures live in a buffer kept under that key, and the next forward of the same view
        reads them as a scheduling hint (deepest blocks first) and -- depthCuts -- bins every tile only as deep as
        that visit needed it plus a margin (gs_set_view_hints).  A forward under cuts may MISS (a tile needed more
        than it was given): outputs are final only once forwardMissed() said False; renderChecked() does both."""
        cam = camera if isinstance(camera, _lib.gs_camera) else self._camera(
            camera.worldViewTransform, camera.projectionMatrix, camera.cameraCenter, camera.FoVx, camera.FoVy,
            camera.focalX, camera.focalY)
        model = getattr(camera, "model", "pinhole")      # (the camera's model: views of both kinds share a renderer)
        if model != self._camera_model:
            self.setCameraModel(model)
        p = {k: (v if isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.float32 and v.is_contiguous()
                 else self._t(v)) for k, v in params.items()}
        N = p["xyz"].shape[0]
        K = 1 + p["features_rest"].shape[1]
        P = self.W * self.H
        if getattr(self, "_fbuf", None) is None:
            self._fbuf = (self._empty(P, 3), self._empty(P), self._empty(P))
        color, depth, alpha = self._fbuf
        radii = self._empty(N) if want_radii else None
        buf = None
        if viewKey is not None and self._hints_ok:
            buf = self._work_hints.get(viewKey)
            if buf is None:
                n = C.c_int()
                self._check(self.lib.gs_view_hint_words(self.ctx, C.byref(n)))
                buf = self._work_hints[viewKey] = torch.zeros(n.value, dtype=torch.int32, device=self.device)
        self._check(self.lib.gs_set_view_hints(self.ctx, _p(buf), 0 if buf is None else int(buf.numel())))   # hint in, measurement out
        # per-view policy: cuts only where they pay (CutPolicy)
        use = False
        if buf is not None:
            pol = self._cut_policy.get(viewKey)
            if pol is None:
                pol = self._cut_policy[viewKey] = CutPolicy(self.cutMinDropped, self.cutProbeInterval)
            pol.min_dropped, pol.probe_interval = self.cutMinDropped, self.cutProbeInterval
            use = pol.begin(depthCuts and self.depthCuts)
        self._cut_view = viewKey if use else None
        self._hinted_view = viewKey if buf is not None else None     # whose cuts the backward of this forward renews
        self._check(self.lib.gs_set_depth_cuts(self.ctx, 1 if use else 0))
        self._check(self.lib.gs_render_forward(self.ctx, N, K, _p(p["xyz"]), _p(p["features_dc"]),
                                               _p(p["features_rest"]), _p(p["scales"]), _p(p["rotation"]),
                                               _p(p["opacity"]), C.byref(cam), _p(color),
                                               _p(depth if wantDepth else None), _p(alpha), _p(radii)))
        # (radii: the backward of a forward made under setADCStats reads the caller's radii buffer -- it lives until the next forward)
        self._fused = dict(params=p, color=color, depth=depth if wantDepth else None, alpha=alpha, radii=radii)
        return RenderResult(color.view(self.H, self.W, 3), depth.view(self.H, self.W, 1) if wantDepth else None,
                            alpha.view(self.H, self.W, 1), None if radii is None else radii > 0, radii)

    def dropDepthCuts(self):
        """Forget every view's depth cuts (after the model was rebuilt): the next forward of each view bins in full
        and the cuts are derived afresh.  The scheduling hints stay.  Host-side only: a view whose policy says "no cuts yet"
        never bins under the words its buffer still holds (CutPolicy.begin), and the backward preparation of its next forward
        rewrites every one of them -- clearing the buffers on the device as well (round 3) was one memset launch per view, a
        hundred per densify event."""
        for pol in self._cut_policy.values():
            pol.cuts_cleared()

    def _cuts_renewed(self):
        """Called where a backward preparation of the last fused forward is queued (its loss or its backward)."""
        if self._hinted_view is not None:
            pol = self._cut_policy.get(self._hinted_view)
            if pol is not None:
                pol.renewed()

    def forwardMissed(self) -> bool:
        """True if the last renderForward ran under depth cuts and has to be repeated with depthCuts=False.  Waits
        for that forward only (work queued behind it keeps the GPU busy meanwhile)."""
        if os.environ.get("GSPLAT_DEBUG_NO_MISS_CHECK"):      # timing experiments only: results are not guaranteed
            return False
        m = C.c_int()
        self._check(self.lib.gs_forward_missed(self.ctx, C.byref(m)))
        if self._cut_view is not None:
            st = (C.c_uint32 * 2)()
            self._check(self.lib.gs_cut_stats(self.ctx, st))
            self._cut_policy[self._cut_view].report(bool(m.value), int(st[0]), int(st[1]))
            self._cut_view = None
        return bool(m.value)

    def renderChecked(self, params: dict, camera, want_radii: bool = False, viewKey=None, wantDepth: bool = True):
        """renderForward, repeated without depth cuts if it missed: outputs are final on return."""
        res = self.renderForward(params, camera, want_radii, viewKey, wantDepth=wantDepth)
        if self.forwardMissed():
            res = self.renderForward(params, camera, want_radii, viewKey, depthCuts=False, wantDepth=wantDepth)
        return res

    @property
    def blockLists(self) -> bool:
        """True when the fused path of this renderer works on block lists (a tile size that is not a multiple of 16: the 16 x 16
        blocks are enumerated per tile and binned, sorted and blended one by one; include/gsplat.h)."""
        return (self.TILE_SIZE.w % 16 != 0 or self.TILE_SIZE.h % 16 != 0) and os.environ.get("GSPLAT_BLOCK_LISTS", "1") != "0"

    def blockWork(self):
        """Sweep length of every pixel block in the last fused forward (list entries up to the block's last contributing one):
        int32 [gs_block_count].  Fused path with 16 x 16 tiles or block lists only."""
        n = C.c_int()
        self._check(self.lib.gs_block_count(self.ctx, C.byref(n)))
        out = self._empty(n.value, dtype=torch.int32)
        self._check(self.lib.gs_copy_block_work(self.ctx, _p(out)))
        return out

    def lastContrib(self):
        out = self._empty(self.H, self.W, dtype=torch.int32)
        self._check(self.lib.gs_copy_last_contrib(self.ctx, _p(out)))
        return out

    STAGES = ("proj_fwd", "bin", "blend_fwd", "loss", "blend_bwd", "proj_bwd", "adam", "distortion_bwd")

    def profile(self, stages=True):
        """stages: True = all, False/None = off, or an iterable of stage names."""
        if stages is True:
            mask = (1 << len(self.STAGES)) - 1
        elif not stages:
            mask = 0
        else:
            mask = sum(1 << self.STAGES.index(s) for s in stages)
        self._check(self.lib.gs_profile_enable(self.ctx, mask))

    def profileRead(self):
        ms, calls = (C.c_float * 8)(), (C.c_int * 8)()
        self._check(self.lib.gs_profile_read(self.ctx, ms, calls))
        return {n: (ms[i], calls[i]) for i, n in enumerate(self.STAGES)}

    def renderBackward(self, cotColor, cotDepth=None, cotAlpha=None, out: dict | None = None):
        p = self._fused["params"]
        g = out or {k: torch.empty_like(v) for k, v in p.items()}
        cotColor = self._t(cotColor)
        cotDepth = None if cotDepth is None else self._t(cotDepth)
        cotAlpha = None if cotAlpha is None else self._t(cotAlpha)
        self._cuts_renewed()
        self._check(self.lib.gs_render_backward(self.ctx, _p(cotColor), _p(cotDepth), _p(cotAlpha), _p(g["xyz"]),
                                                _p(g["features_dc"]), _p(g["features_rest"]), _p(g["scales"]),
                                                _p(g["rotation"]), _p(g["opacity"])))
        return g

    @staticmethod
    def _bound_pair(who, names, a, b, n):
        """The two tensors a setter binds (`names` = what it calls them): both None, or both contiguous float32 device tensors
        of n elements."""
        if (a is None) != (b is None):
            raise ValueError(f"{who}: {names} are both given or both None")
        for t in (a, b):
            if t is not None and (t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous() or t.device.type != "cuda"):
                raise ValueError(f"{who}: {names} are contiguous float32 device tensors of {n} elements")

    def setPoseCorrection(self, delta=None, grad=None):
        """gs_set_pose_correction: delta / grad float32 device tensors of 6 elements (w, tau), or both None (off, the default).
        The following renderForward renders the camera c2w [[R(w), tau], [0, 1]] (camera.apply_pose_correction), and its
        renderBackward / renderBackwardAdam overwrite grad with dL/d delta."""
        self._bound_pair("setPoseCorrection", "delta and grad", delta, grad, 6)
        self._check(self.lib.gs_set_pose_correction(self.ctx, None if delta is None else _p(delta), None if grad is None else _p(grad)))
        self._pose = (delta, grad)        # (kept alive while the library holds their addresses)

    @property
    def poseCorrection(self):
        """(delta, grad) as setPoseCorrection last bound them, (None, None) when off."""
        return getattr(self, "_pose", (None, None))

    def setExposure(self, M=None, grad=None):
        """gs_set_exposure: M / grad float32 device tensors of 12 elements (M = [A | b] row-major 3 x 4), or both None (off, the
        default).  The following lossForwardBackward calls take the loss of A render + b, return dL/d render as the colour
        cotangent and overwrite grad with dL/dM (include/gsplat.h)."""
        self._bound_pair("setExposure", "M and grad", M, grad, 12)
        self._check(self.lib.gs_set_exposure(self.ctx, _p(M), _p(grad)))
        self._exposure = (M, grad)        # (kept alive while the library holds their addresses)

    def applyExposure(self, img, M, out=None):
        """gs_apply_exposure: A img + b per pixel of an [..., 3] image (a new tensor; out=img works in place)."""
        img, M = self._t(img), self._t(M)
        if img.shape[-1] != 3 or M.numel() != 12:
            raise ValueError("applyExposure: an [..., 3] image and a 12-element M")
        out = torch.empty_like(img) if out is None else out
        if out.shape != img.shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("applyExposure: out is a contiguous float32 tensor of the image's shape")
        self._check(self.lib.gs_apply_exposure(self.ctx, img.numel() // 3, _p(M), _p(img), _p(out)))
        return out

    def undistortImage(self, img, lens, dstK=None, dstSize=None, mode: str = "color", wantValid: bool = True):
        """gs_undistort: (out, valid) device tensors -- the image seen through `lens` (lens.LensModel) resampled into the pinhole
        dstK = (fx, fy, cx, cy) of size dstSize = (W, H); None: the lens's own fx, fy, cx, cy and the source's size.  mode
        "color": float32 [H, W, C], C in 1 .. 4 (or [H, W]); "mask": uint8 [H, W]; "depth": float32 [H, W], 0 = hole.  valid is
        uint8 [H, W], 255 where the four taps lie in the source and the lens has not folded back (None with wantValid=False).
        What lens.undistort_image states in float64; a loader's `undistorter` (data.py)."""
        from . import lens as _lens
        if mode not in _lens.MODES:
            raise ValueError(f"undistortImage: mode is one of {sorted(_lens.MODES)}")
        dtype = torch.uint8 if mode == "mask" else torch.float32
        if not isinstance(img, torch.Tensor):
            img = torch.from_numpy(np.ascontiguousarray(img))
        if mode == "mask" and img.dtype != torch.uint8:
            raise ValueError("undistortImage: a mask is uint8 [H, W]")
        src = img.to(device=self.device, dtype=dtype).contiguous()
        if src.dim() not in (2, 3) or (src.dim() == 3 and (mode != "color" or not 1 <= src.shape[2] <= 4)):
            raise ValueError("undistortImage: a colour image is [H, W, C] with C in 1 .. 4, a mask or a depth [H, W]")
        srcH, srcW = int(src.shape[0]), int(src.shape[1])
        chans = int(src.shape[2]) if src.dim() == 3 else 1
        nfx, nfy, ncx, ncy = (float(v) for v in (lens.K if dstK is None else dstK))
        W, H = (srcW, srcH) if dstSize is None else (int(dstSize[0]), int(dstSize[1]))
        if W < 1 or H < 1:
            raise ValueError("undistortImage: dstSize = (width, height), both positive")
        fisheye = isinstance(lens, _lens.FisheyeLensModel)      # (k1 .. k4 into the equidistant camera: gs_undistort_fisheye)
        L = (_lib.gs_fisheye_lens if fisheye else _lib.gs_lens)(*lens.K, *lens.coefficients, nfx, nfy, ncx, ncy)
        out = torch.empty((H, W) + tuple(src.shape[2:]), dtype=dtype, device=self.device)
        valid = torch.empty((H, W), dtype=torch.uint8, device=self.device) if wantValid else None
        call = self.lib.gs_undistort_fisheye if fisheye else self.lib.gs_undistort
        self._check(call(self.ctx, C.byref(L), srcW, srcH, W, H, chans, _lens.MODES[mode], _p(src), _p(out), _p(valid)))
        return out, valid

    def undistortFisheyeImage(self, img, lens, dstK=None, dstSize=None, mode: str = "color", wantValid: bool = True):
        """gs_undistort_fisheye: undistortImage for a lens.FisheyeLensModel -- the view resampled into the ideal equidistant
        camera dstK = (fx, fy, cx, cy) that Camera(model="fisheye") renders (None: the lens's own intrinsics and the source's
        size).  Modes, shapes and the validity output are undistortImage's; lens.undistort_fisheye_image states it in float64."""
        from . import lens as _lens
        if not isinstance(lens, _lens.FisheyeLensModel):
            raise ValueError("undistortFisheyeImage takes a lens.FisheyeLensModel")
        return self.undistortImage(img, lens, dstK, dstSize, mode, wantValid)

    @staticmethod
    def _grid_shape(shape, what):
        try:
            gw, gh, gl = (int(x) for x in shape)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: shape = (grid_w, grid_h, grid_l)") from None
        if not (2 <= gw <= 64 and 2 <= gh <= 64 and 2 <= gl <= 32) or tuple(shape) != (gw, gh, gl):
            raise ValueError(f"{what}: shape = (grid_w, grid_h, grid_l) with 2 <= grid_w, grid_h <= 64 and 2 <= grid_l <= 32")
        return gw, gh, gl

    def setBilateralGrid(self, grid=None, grad=None, shape=(16, 16, 8), tv_weight: float = 10.0):
        """gs_set_bilateral_grid: grid / grad float32 device tensors of grid_h x grid_w x grid_l x 12 elements (shape = (grid_w,
        grid_h, grid_l); G[y][x][z] holds a 12-float M = [A | b] as in setExposure), or both None (off, the default).  The
        following lossForwardBackward calls take the loss of the render under the grid, return dL/d render as the colour
        cotangent and overwrite grad with dL/dG plus tv_weight times the TV term's gradient (include/gsplat.h).  Exclusive with
        setExposure."""
        gw, gh, gl = self._grid_shape(shape, "setBilateralGrid")
        tv = float(tv_weight)
        if not (math.isfinite(tv) and tv >= 0.0):
            raise ValueError("setBilateralGrid: tv_weight must be finite and >= 0")
        self._bound_pair("setBilateralGrid", "grid and grad", grid, grad, gw * gh * gl * 12)
        self._check(self.lib.gs_set_bilateral_grid(self.ctx, _p(grid), _p(grad), gw, gh, gl, C.c_float(tv)))
        self._bilateral = (grid, grad)    # (kept alive while the library holds their addresses)

    def applyBilateralGrid(self, img, grid, shape=(16, 16, 8), out=None):
        """gs_apply_bilateral_grid: an [H, W, 3] image under the grid (a new tensor; out=img works in place)."""
        img, grid = self._t(img), self._t(grid)
        gw, gh, gl = self._grid_shape(shape, "applyBilateralGrid")
        if img.dim() != 3 or img.shape[-1] != 3 or grid.numel() != gw * gh * gl * 12:
            raise ValueError("applyBilateralGrid: an [H, W, 3] image and a grid of grid_h x grid_w x grid_l x 12 elements")
        out = torch.empty_like(img) if out is None else out
        if out.shape != img.shape or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("applyBilateralGrid: out is a contiguous float32 tensor of the image's shape")
        H, W = int(img.shape[0]), int(img.shape[1])
        self._check(self.lib.gs_apply_bilateral_grid(self.ctx, W, H, _p(grid), gw, gh, gl, _p(img), _p(out)))
        return out

    # -- per-pixel loss mask (include/gsplat.h gs_set_loss_mask; loss_mask.py restates it) --------------
    def setLossMask(self, mask=None):
        """gs_set_loss_mask: a uint8 (weight v / 255; 255 keeps a pixel, 0 ignores it) or bool (0 / 255) image of shape (H, W),
        tensor or array, or None (off, the default).  The following lossForwardBackward calls take the loss of the weighted
        render and target -- after a bound exposure or bilateral grid -- normalised over all pixels as without a mask (no
        division by the mask's coverage), and return w * dL/d(w render) as the colour cotangent: exactly zero where the mask is.
        A contiguous uint8 device tensor is bound as it is (write it in place and the next loss sees it); anything else is
        converted and uploaded once, here."""
        if mask is None:
            self._check(self.lib.gs_set_loss_mask(self.ctx, None))
            self._loss_mask = None
            return
        loss_mask.validate(mask, self.H, self.W, "setLossMask")
        if not torch.is_tensor(mask):
            mask = torch.from_numpy(np.ascontiguousarray(loss_mask.as_uint8(mask)))
        if mask.dtype == torch.bool:
            mask = mask.to(torch.uint8) * 255
        mask = mask.to(self.device).contiguous()
        self._check(self.lib.gs_set_loss_mask(self.ctx, _p(mask)))
        self._loss_mask = mask            # (kept alive while the library holds its address)

    @property
    def lossMask(self):
        """The bound mask as the uint8 device tensor the library reads, or None."""
        return self._loss_mask

    @lossMask.setter
    def lossMask(self, mask):
        self.setLossMask(mask)

    def setAntialiased(self, enable: bool = True):
        """gs_set_antialiasing: the anti-aliased mode (Mip-Splatting's 2-D filter; include/gsplat.h) for the
        following renderForward calls, off by default.  Every backward uses the mode of its forward, so a GaussianTrainer
        trains in whatever mode its renderer is in.  All ranks of a data-parallel job must agree (a rank that does not shows
        up as a replica mismatch).  PLY snapshots do not record the mode: render a model in the mode it was trained in."""
        self._check(self.lib.gs_set_antialiasing(self.ctx, 1 if enable else 0))
        self._antialiased = bool(enable)

    def setCameraModel(self, model: str = "pinhole"):
        """gs_set_camera_model: "pinhole" (the default) or "fisheye", the ideal equidistant camera (include/gsplat.h, DESIGN.md
        section 29), for the following forwards; every fused backward uses the model of its forward.  renderForward and
        renderChecked set it from their camera (`camera.model`, "pinhole" for a camera without one), so a trainer follows its
        cameras; projectionScreenFused* and forwardWithCameraParams* take plain matrices and use the setting in effect.
        Not with a pose correction, a 3-D filter or the data-parallel entry points: those calls raise."""
        from .camera import CAMERA_MODELS
        if model not in CAMERA_MODELS:
            raise ValueError(f"setCameraModel: model is one of {sorted(CAMERA_MODELS)}")
        self._check(self.lib.gs_set_camera_model(self.ctx, CAMERA_MODELS[model]))
        self._camera_model = model

    def setSHDegree(self, degree: int):
        """gs_set_sh_degree: the active SH degree, 0 .. maxSHDegree, of the following forwards (include/gsplat.h, DESIGN.md section
        30); the default is the maximum, the degree the renderer was built with.  K of the model stays the row stride: only the
        bands k < (degree + 1)^2 are evaluated, and the gradient of every other coefficient is an exact zero.  Every fused
        backward uses the degree of its forward.  active_sh_degree stays what the constructor got (callers size K from it)."""
        if isinstance(degree, bool) or int(degree) != degree:
            raise ValueError("setSHDegree: degree is an integer")
        self._check(self.lib.gs_set_sh_degree(self.ctx, int(degree)))
        self._sh_degree = int(degree)

    @property
    def shDegree(self) -> int:
        return self._sh_degree

    @shDegree.setter
    def shDegree(self, degree: int):
        self.setSHDegree(degree)

    @property
    def maxSHDegree(self) -> int:
        return self.active_sh_degree

    @property
    def cameraModel(self) -> str:
        return self._camera_model

    @cameraModel.setter
    def cameraModel(self, model: str):
        self.setCameraModel(model)

    @property
    def antialiased(self) -> bool:
        return self._antialiased

    @antialiased.setter
    def antialiased(self, enable: bool):
        self.setAntialiased(enable)

    # -- background colour (include/gsplat.h gs_set_background; background.py restates it) -------------
    def setBackground(self, rgb=None):
        """gs_set_background: the colour the following renderForward / blendForward calls composite over (three finite floats,
        not confined to [0, 1]), or None (the default): the renderer's own black or white, bit for bit as without the call.
        Every fused backward uses the background of its forward.  A by-value kernel argument: free to change every step."""
        if rgb is None:
            self._check(self.lib.gs_set_background(self.ctx, None))
            self._background = None
            return
        b = np.ascontiguousarray(np.asarray(rgb.detach().cpu() if torch.is_tensor(rgb) else rgb, dtype=np.float32).reshape(-1))
        if b.size != 3:
            raise ValueError("setBackground: three floats (r, g, b), or None")
        self._check(self.lib.gs_set_background(self.ctx, b.ctypes.data_as(C.c_void_p)))
        self._background = b          # (what setBackground last set, as _sparse_adam is kept: a trainer puts it back behind its step)

    @property
    def customBackground(self):
        """What setBackground last set: float32 [3], or None for the renderer's own black or white (`background` is the colour
        in effect either way)."""
        return self._background

    @property
    def background(self):
        """The colour in effect (gs_get_background), float32 [3]: the one set, or the renderer's black or white."""
        b = np.zeros(3, np.float32)
        self._check(self.lib.gs_get_background(self.ctx, b.ctypes.data_as(C.c_void_p)))
        return b

    def compositeTarget(self, rgb, alpha, bg, out=None):
        """gs_composite_target: the target of an RGBA view over bg, fma(a, rgb, (1 - a) bg) per pixel of an [..., 3] straight
        (un-premultiplied) image and its [...] alpha (a new tensor; out=rgb works in place)."""
        rgb, alpha = self._t(rgb), self._t(alpha)
        b = np.ascontiguousarray(np.asarray(bg.detach().cpu() if torch.is_tensor(bg) else bg, dtype=np.float32).reshape(-1))
        if rgb.shape[-1] != 3 or alpha.numel() * 3 != rgb.numel() or b.size != 3:
            raise ValueError("compositeTarget: an [..., 3] image, its [...] alpha and three background floats")
        out = torch.empty_like(rgb) if out is None else out
        if out.shape != rgb.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != rgb.device:
            raise ValueError("compositeTarget: out is a contiguous float32 device tensor of the image's shape")
        self._check(self.lib.gs_composite_target(self.ctx, alpha.numel(), _p(rgb), _p(alpha), b.ctypes.data_as(C.c_void_p),
                                                 _p(out)))
        return out

    # -- AbsGS densification statistic (include/gsplat.h gs_set_absgrad; absgrad.py restates it) --------
    def setAbsgrad(self, enable: bool = True):
        """gs_set_absgrad: the following renderBackward / fused train steps also sum, per Gaussian, the per-pixel absolute values
        of the 2-D mean gradient (absgrad()), and a grad-norm accumulator gets hypot(W/2 Ax, H/2 Ay) in place of |grad xyz|.
        Single-device steps; refused on a renderer whose tile size is served by the generic blend kernels.  Off (the
        default): no kernel, buffer or result differs."""
        self._check(self.lib.gs_set_absgrad(self.ctx, 1 if enable else 0))
        self._absgrad = bool(enable)

    def absgrad(self):
        """gs_get_absgrad: (Ax, Ay) [N, 2] of the last backward, in pixel units; valid until the next forward or backward."""
        if getattr(self, "_fused", None) is None:
            raise GsplatError(5, "absgrad: no renderForward on this renderer")
        N = int(self._fused["params"]["xyz"].shape[0])
        out = self._empty(N, 2)
        self._check(self.lib.gs_get_absgrad(self.ctx, N, _p(out)))
        return out

    # -- adaptive density control (include/gsplat.h gs_set_adc_stats; adc.py states the rule) -------------
    _ADC_ORDER = ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")

    def setADCStats(self, gradSum=None, count=None, maxRadius=None):
        """gs_set_adc_stats: the following renderBackward / fused train steps add, for every Gaussian their forward saw,
        hypot(W/2 gx, H/2 gy) of its 2-D mean gradient to gradSum, 1 to count and the radius into maxRadius's running maximum
        (float32 [N] on the device, all three or none; they must stay alive while set).  Single-device steps; refused on a
        renderer whose tile size is served by the generic blend kernels.  None (the default): no kernel, buffer or result differs."""
        self._check(self.lib.gs_set_adc_stats(self.ctx, _p(gradSum), _p(count), _p(maxRadius)))
        self._adc_stats = None if gradSum is None else (gradSum, count, maxRadius)

    @property
    def adcStats(self):
        """(gradSum, count, maxRadius) as setADCStats last set them, or None."""
        return getattr(self, "_adc_stats", None)

    def adcAccumulate(self, rows16, radii, useAbs: bool, gradSum, count, maxRadius):
        """gs_adc_accumulate: the step's statistic kernel on the caller's rows [N, 16] and radii [N], in place."""
        rows16, radii = self._t(rows16), self._t(radii)
        self._check(self.lib.gs_adc_accumulate(self.ctx, int(radii.shape[0]), _p(rows16), _p(radii), int(bool(useAbs)),
                                               _p(gradSum), _p(count), _p(maxRadius)))

    def adcClassify(self, gradSum, count, maxRadius, scales, opacity, gradThreshold=0.0002, percentDense=0.01, minOpacity=0.005,
                    maxScreenSize=20.0, pruneWorld=0.1, sceneExtent=1.0, allowDensify=True, sizePrune=False):
        """gs_adc_classify: (actions, counts) int32 [N] in classifyGaussians' words."""
        gradSum, count, maxRadius = self._t(gradSum), self._t(count), self._t(maxRadius)
        scales, opacity = self._t(scales), self._t(opacity)
        N = int(gradSum.shape[0])
        actions, counts = self._empty(N, dtype=torch.int32), self._empty(N, dtype=torch.int32)
        prm = _lib.gs_adc_params(float(gradThreshold), float(percentDense), float(minOpacity), float(maxScreenSize),
                                 float(pruneWorld), float(sceneExtent))
        self._check(self.lib.gs_adc_classify(self.ctx, N, _p(gradSum), _p(count), _p(maxRadius), _p(scales),
                                             int(scales.shape[1]) if N else 3, _p(opacity), C.byref(prm),
                                             int(bool(allowDensify)), int(bool(sizePrune)), _p(actions), _p(counts)))
        return actions, counts

    def adcGather(self, params: dict, gather, noiseMode, noise, revisedOpacity: bool = False, out: dict | None = None):
        """gs_adc_gather: densifyGather's sibling -- split children sampled from the Gaussian, clones copied exactly."""
        p = {k: self._t(v) for k, v in params.items()}
        total, K = int(gather.shape[0]), int(p["features_rest"].shape[1]) + 1
        o = out or {k: self._empty(total, *v.shape[1:]) for k, v in p.items()}
        self._check(self.lib.gs_adc_gather(self.ctx, total, K, _p(p["xyz"]), _p(p["features_dc"]), _p(p["features_rest"]),
                                           _p(p["scales"]), _p(p["rotation"]), _p(p["opacity"]), _p(gather), _p(noiseMode),
                                           _p(self._t(noise)), int(bool(revisedOpacity)), _p(o["xyz"]), _p(o["features_dc"]),
                                           _p(o["features_rest"]), _p(o["scales"]), _p(o["rotation"]), _p(o["opacity"])))
        return o

    def adcGatherMoments(self, moments: dict, gather, noiseMode, actions, out: dict | None = None):
        """gs_adc_gather_moments on one moment arena's six tensors (a dict keyed like the parameters): kept rows and clone
        originals copied bit for bit, split children and clone copies zero."""
        mo = {k: self._t(v) for k, v in moments.items()}
        total, K = int(gather.shape[0]), int(mo["features_rest"].shape[1]) + 1
        o = out or {k: self._empty(total, *v.shape[1:]) for k, v in mo.items()}
        tin = (C.c_void_p * 6)(*[_p(mo[k]) for k in self._ADC_ORDER])
        tout = (C.c_void_p * 6)(*[_p(o[k]) for k in self._ADC_ORDER])
        self._check(self.lib.gs_adc_gather_moments(self.ctx, total, K, _p(gather), _p(noiseMode), _p(actions), tin, tout))
        return o

    def adcResetOpacity(self, opacity, mOpacity, vOpacity, resetValue: float = 0.01):
        """gs_adc_reset_opacity, in place: opacity = min(opacity, logit(resetValue)); the segment's two moments zeroed."""
        self._check(self.lib.gs_adc_reset_opacity(self.ctx, int(opacity.numel()), _p(opacity), _p(mOpacity), _p(vOpacity),
                                                  C.c_float(resetValue)))

    # -- sparse Adam (include/gsplat.h gs_set_sparse_adam; sparse_adam.py restates the rule) ---------------
    def setSparseAdam(self, enable: bool = True):
        """gs_set_sparse_adam: the following renderForward calls keep which Gaussians they gave a radius > 0 (visibility()), and
        renderBackwardAdam / adamStepVisible update those rows alone: every element of an invisible row -- parameter and both
        moments -- keeps its bits.  Single-device steps; not with the MCMC strategy or a 3-D filter.  Off (the default): no
        kernel, buffer or result differs."""
        self._check(self.lib.gs_set_sparse_adam(self.ctx, 1 if enable else 0))
        self._sparse_adam = bool(enable)

    @property
    def sparseAdam(self) -> bool:
        return self._sparse_adam

    def visibility(self):
        """gs_get_visibility: torch.bool [N], the Gaussians the last renderForward made under setSparseAdam saw (radius > 0)."""
        if getattr(self, "_fused", None) is None:
            raise GsplatError(5, "visibility: no renderForward on this renderer")
        N = int(self._fused["params"]["xyz"].shape[0])
        out = self._empty(max(N, 1), dtype=torch.uint8)[:N]
        self._check(self.lib.gs_get_visibility(self.ctx, N, _p(out)))
        return out.bool()

    def adamStepVisible(self, arena, grad, m, v, seg_end, lrs, seg_row_floats, N: int, visible=None, beta1=0.9, beta2=0.999,
                        eps=1e-15, grad_scale=1.0):
        """gs_adam_step_visible: gs_adam_step on the rows < N whose mask byte is set (visible: torch.bool / uint8 [N] on the
        device, or None for the mask of the last renderForward made under setSparseAdam).  seg_end / lrs / seg_row_floats: one
        entry per segment (a GaussModel's seg_end, arenaLearningRates and sparse_adam.model_row_floats)."""
        k = len(seg_end)
        if len(lrs) != k or len(seg_row_floats) != k:
            raise ValueError("adamStepVisible: one learning rate and one row width per segment")
        vis = None
        if visible is not None:
            vis = visible.to(device=self.device, dtype=torch.uint8).contiguous()
            if vis.numel() != int(N):
                raise ValueError("adamStepVisible: visible holds N entries")
        self._check(self.lib.gs_adam_step_visible(
            self.ctx, int(arena.numel()), _p(arena), _p(grad), _p(m), _p(v), k, (C.c_longlong * k)(*[int(x) for x in seg_end]),
            (C.c_float * k)(*[float(x) for x in lrs]), (C.c_int * k)(*[int(x) for x in seg_row_floats]), C.c_float(beta1),
            C.c_float(beta2), C.c_float(eps), C.c_float(grad_scale), int(N), _p(vis)))

    # -- the 3-D smoothing filter (include/gsplat.h gs_set_filter3d; filter3d.py restates it in float64) ---
    def setFilterCameras(self, cameras):
        """gs_set_filter3d_cameras: the training cameras computeFilter3D measures against (Camera objects or gs_camera structs;
        an empty list frees the table)."""
        cams = [c if isinstance(c, _lib.gs_camera) else self._camera(c.worldViewTransform, c.projectionMatrix, c.cameraCenter,
                                                                      c.FoVx, c.FoVy, c.focalX, c.focalY) for c in cameras]
        arr = (_lib.gs_camera * max(len(cams), 1))(*cams)
        self._check(self.lib.gs_set_filter3d_cameras(self.ctx, len(cams), C.cast(arr, C.c_void_p) if cams else None))
        self._filter_cameras = len(cams)

    def computeFilter3D(self, xyz, out=None):
        """gs_compute_filter3d: the filter widths [N] of the positions xyz [N, 3] (into out[:N] when given: a contiguous float32
        device tensor of at least N elements; nothing is allocated then).  Asynchronous."""
        xyz = xyz if isinstance(xyz, torch.Tensor) and xyz.is_cuda and xyz.dtype == torch.float32 and xyz.is_contiguous() else self._t(xyz)
        N = int(xyz.shape[0])
        if out is None:
            out = self._empty(N)
        if out.dtype != torch.float32 or not out.is_contiguous() or out.device.type != "cuda" or out.numel() < N:
            raise ValueError("computeFilter3D: out is a contiguous float32 device tensor of at least N elements")
        self._check(self.lib.gs_compute_filter3d(self.ctx, N, _p(xyz), _p(out)))
        return out

    def setFilter3D(self, t=None):
        """gs_set_filter3d: the filter widths (a contiguous float32 device tensor of at least N elements) of the following
        renderForward calls, or None (off, the default).  A backward uses the filter of its forward: keep the tensor unchanged
        between the two.  Single-device steps and the reference strategy only."""
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != "cuda"):
            raise ValueError("setFilter3D: a contiguous float32 device tensor, or None")
        self._check(self.lib.gs_set_filter3d(self.ctx, _p(t)))
        self._filter3d = t                # (kept alive while the library holds its address)

    @property
    def filter3D(self):
        return getattr(self, "_filter3d", None)

    def bakeFilter3D(self, params: dict, filter=None):
        """gs_filter3d_bake: a copy of params with scales = log(s_eff) and opacity = logit(sigma kappa) under `filter` (default:
        the filter that is set).  Rendered with the filter off, the baked model is the filtered one."""
        f = self.filter3D if filter is None else filter
        if f is None:
            raise ValueError("bakeFilter3D: no filter is set and none was given")
        sc, op = self._t(params["scales"]), self._t(params["opacity"])
        N = int(sc.shape[0])
        if f.numel() < N or op.numel() != N:
            raise ValueError("bakeFilter3D: the filter holds fewer than N widths")
        out = dict(params)
        out["scales"], out["opacity"] = torch.empty_like(sc), torch.empty_like(op)
        self._check(self.lib.gs_filter3d_bake(self.ctx, N, _p(sc), _p(op), _p(f), _p(out["scales"]), _p(out["opacity"])))
        return out

    # -- the MCMC strategy (include/gsplat.h gs_set_mcmc; mcmc.MCMCConfig.params builds the gs_mcmc_params) -----------------
    def setMCMC(self, params=None):
        """gs_set_mcmc: the MCMC strategy's per-step part (regularisers, noise) in the following renderBackwardAdam calls, or
        None (off, the default)."""
        self._check(self.lib.gs_set_mcmc(self.ctx, None if params is None else C.byref(params)))
        self._mcmc = params

    @property
    def mcmc(self):
        """The gs_mcmc_params setMCMC last set, or None."""
        return getattr(self, "_mcmc", None)

    def mcmcRegularizerGrad(self, scales, opacity, gradScales, gradOpacity, params):
        """gs_mcmc_regularizer_grad: gradOpacity / gradScales += the regularisers' gradients (in place)."""
        N = int(scales.shape[0])
        self._check(self.lib.gs_mcmc_regularizer_grad(self.ctx, N, _p(scales), _p(opacity), _p(gradScales), _p(gradOpacity),
                                                      C.byref(params)))

    def mcmcInjectNoise(self, xyz, scales, rotation, opacity, lr_xyz: float, params):
        """gs_mcmc_inject_noise: xyz += the step's noise (in place; gated like the optimizer kernels)."""
        N = int(xyz.shape[0])
        self._check(self.lib.gs_mcmc_inject_noise(self.ctx, N, _p(xyz), _p(scales), _p(rotation), _p(opacity),
                                                  C.c_float(lr_xyz), C.byref(params)))

    def mcmcRandom(self, seed: int, iteration: int, stream: int, n: int):
        """gs_mcmc_random: (words uint32 [n,4] as int32, normals [n,3], uniforms float64 [n]) of stream 0 noise / 1 relocation
        draws / 2 growth draws."""
        words = self._empty(max(n, 1), 4, dtype=torch.int32)[:n]
        normals = self._empty(max(n, 1), 3)[:n]
        uniforms = self._empty(max(n, 1), dtype=torch.float64)[:n]
        self._check(self.lib.gs_mcmc_random(self.ctx, C.c_ulonglong(int(seed)).value, int(iteration), int(stream), int(n),
                                            _p(words), _p(normals), _p(uniforms)))
        return words, normals, uniforms

    def _mcmc_rows(self, params: dict):
        K = int(params["features_rest"].shape[1]) + 1
        return K, [_p(params[k]) for k in ("xyz", "features_dc", "features_rest", "scales", "rotation", "opacity")]

    def mcmcRelocate(self, params: dict, arena, m, v, mcmcParams) -> dict:
        """gs_mcmc_relocate over the rows of `params` (views into arena; m / v its moment arenas).  Waits for the counts."""
        K, t = self._mcmc_rows(params)
        st = (C.c_longlong * 4)()
        self._check(self.lib.gs_mcmc_relocate(self.ctx, int(params["xyz"].shape[0]), K, *t, _p(arena), _p(m), _p(v),
                                              C.byref(mcmcParams), st))
        return dict(dead=int(st[0]), relocated=int(st[1]), live=int(st[2]), N=int(st[3]))

    def mcmcGrow(self, params: dict, capacity: int, arena, m, v, mcmcParams) -> int:
        """gs_mcmc_grow: appends the grown rows behind the N rows of `params` (each tensor must have room for `capacity`
        rows); returns the new count.  Waits for the counts."""
        K, t = self._mcmc_rows(params)
        n = C.c_int()
        self._check(self.lib.gs_mcmc_grow(self.ctx, int(params["xyz"].shape[0]), int(capacity), K, *t, _p(arena), _p(m), _p(v),
                                          C.byref(mcmcParams), C.byref(n)))
        return int(n.value)

    def renderBackwardAdam(self, cotColor, arena, m, v, lrs, beta1=0.9, beta2=0.999, eps=1e-15, grad_scale=1.0,
                           cotDepth=None, cotAlpha=None):
        """Backward with the Adam step fused into the projection backward (single-device steps): the parameters the
        preceding renderForward saw must be views into `arena`; m / v are the moment arenas of the same layout; lrs
        in the reference's parameter order (xyz, f_dc, f_rest, scales, rotation, opacity).  No gradient arena is
        written."""
        cotColor = self._t(cotColor)
        cotDepth = None if cotDepth is None else self._t(cotDepth)
        cotAlpha = None if cotAlpha is None else self._t(cotAlpha)
        lr = (C.c_float * 6)(*[float(x) for x in lrs])
        self._cuts_renewed()
        self._check(self.lib.gs_render_backward_adam(self.ctx, _p(cotColor), _p(cotDepth), _p(cotAlpha), _p(arena), _p(m),
                                                     _p(v), int(arena.numel()), lr, C.c_float(beta1), C.c_float(beta2),
                                                     C.c_float(eps), C.c_float(grad_scale)))

    def renderBackwardDP(self, cotColor, cotDepth=None, cotAlpha=None, out: dict | None = None, colorCot=None):
        """Data-parallel backward: as renderBackward, but returns colorCot[N,3] (colour cotangent after the max(.,0)
        gate) instead of the two SH gradient tensors; see shGradFromViews."""
        p = self._fused["params"]
        g = out or {k: torch.empty_like(p[k]) for k in ("xyz", "scales", "rotation", "opacity")}
        N = p["xyz"].shape[0]
        colorCot = self._empty(N, 3) if colorCot is None else colorCot
        cotColor = self._t(cotColor)
        cotDepth = None if cotDepth is None else self._t(cotDepth)
        cotAlpha = None if cotAlpha is None else self._t(cotAlpha)
        self._cuts_renewed()
        self._check(self.lib.gs_render_backward_dp(self.ctx, _p(cotColor), _p(cotDepth), _p(cotAlpha), _p(g["xyz"]),
                                                   _p(g["scales"]), _p(g["rotation"]), _p(g["opacity"]), _p(colorCot)))
        return g, colorCot

    def shGradFromViewsAdam(self, params: dict, colorCotAll, camCenters, arena, m, v, lr_dc, lr_rest, grad_scale,
                            beta1=0.9, beta2=0.999, eps=1e-15):
        """shGradFromViews + the Adam step of features_dc / features_rest in one pass (they are views into arena).
        Uses params["xyz"] as it is: run it before the geometry slice's Adam step."""
        R, N = int(colorCotAll.shape[0]), int(params["xyz"].shape[0])
        K = int(params["features_rest"].shape[1]) + 1
        cc = np.ascontiguousarray(camCenters, np.float32).reshape(R, 3)
        self._check(self.lib.gs_sh_grad_from_views_adam(
            self.ctx, N, K, R, _p(params["xyz"]), _p(colorCotAll), cc.ctypes.data_as(C.c_void_p), _p(params["features_dc"]),
            _p(params["features_rest"]), _p(arena), _p(m), _p(v), int(arena.numel()), C.c_float(lr_dc), C.c_float(lr_rest),
            C.c_float(beta1), C.c_float(beta2), C.c_float(eps), C.c_float(grad_scale)))

    def renderBackwardDPBegin(self, cotColor, cotDepth=None, cotAlpha=None, colorCot=None):
        """First half of renderBackwardDP: blend backward + colorCot, so the caller can start exchanging colorCot
        while renderBackwardDPFinish (projection backward, the four geometry gradients) runs."""
        N = self._fused["params"]["xyz"].shape[0]
        colorCot = self._empty(N, 3) if colorCot is None else colorCot
        cotColor = self._t(cotColor)
        cotDepth = None if cotDepth is None else self._t(cotDepth)
        cotAlpha = None if cotAlpha is None else self._t(cotAlpha)
        self._cuts_renewed()
        self._check(self.lib.gs_render_backward_dp_begin(self.ctx, _p(cotColor), _p(cotDepth), _p(cotAlpha), _p(colorCot)))
        return colorCot

    def renderBackwardDPFinish(self, out: dict | None = None):
        p = self._fused["params"]
        g = out or {k: torch.empty_like(p[k]) for k in ("xyz", "scales", "rotation", "opacity")}
        self._check(self.lib.gs_render_backward_dp_finish(self.ctx, _p(g["xyz"]), _p(g["scales"]), _p(g["rotation"]),
                                                          _p(g["opacity"])))
        return g

    def renderBackwardDPFinishGeom(self, out: dict, xyzOwn):
        """Round 6 (ABI 6): renderBackwardDPFinish without the SH rows -- out["xyz"] lacks the view-direction term of the xyz
        gradient (shGradFromViewsAdamDir rebuilds it for all views), xyzOwn [N,3] receives a copy of it for the densify statistic."""
        self._check(self.lib.gs_render_backward_dp_finish_geom(self.ctx, _p(out["xyz"]), _p(out["scales"]), _p(out["rotation"]),
                                                               _p(out["opacity"]), _p(xyzOwn)))
        return out

    def renderBackwardDPGeom(self, cotColor, colorCot, out: dict, xyzOwn, cotDepth=None, cotAlpha=None):
        """renderBackwardDPBegin + renderBackwardDPFinishGeom with one kernel behind the blend backward (gs_render_backward_dp_geom)."""
        cotColor = self._t(cotColor)
        cotDepth = None if cotDepth is None else self._t(cotDepth)
        cotAlpha = None if cotAlpha is None else self._t(cotAlpha)
        self._cuts_renewed()
        self._check(self.lib.gs_render_backward_dp_geom(self.ctx, _p(cotColor), _p(cotDepth), _p(cotAlpha), _p(colorCot), _p(out["xyz"]),
                                                        _p(out["scales"]), _p(out["rotation"]), _p(out["opacity"]), _p(xyzOwn)))
        return out

    def shGradFromViewsAdamDir(self, params: dict, colorCotAll, camCenters, ownXyz, arena, m, v, lr_dc, lr_rest, grad_scale, xyzAdd,
                               beta1=0.9, beta2=0.999, eps=1e-15):
        """shGradFromViewsAdam + xyzAdd = the sum over the R views of the xyz gradient's view-direction term + the densify
        statistic of the views this rank rendered (ownXyz: R entries, the xyzOwn tensor of renderBackwardDPFinishGeom for this
        rank's views, None for the others)."""
        R, N = int(colorCotAll.shape[0]), int(params["xyz"].shape[0])
        K = int(params["features_rest"].shape[1]) + 1
        cc = np.ascontiguousarray(camCenters, np.float32).reshape(R, 3)
        own = (C.c_void_p * R)(*[None if t is None else t.data_ptr() for t in ownXyz])
        self._check(self.lib.gs_sh_grad_from_views_adam_dir(
            self.ctx, N, K, R, _p(params["xyz"]), _p(colorCotAll), cc.ctypes.data_as(C.c_void_p), own, _p(params["features_dc"]),
            _p(params["features_rest"]), _p(arena), _p(m), _p(v), int(arena.numel()), C.c_float(lr_dc), C.c_float(lr_rest),
            C.c_float(beta1), C.c_float(beta2), C.c_float(eps), C.c_float(grad_scale), _p(xyzAdd)))

    def shGradFromViews(self, xyz, colorCotAll, camCenters, K: int, out: dict | None = None):
        """grad features_dc / features_rest summed over the R views whose colorCot[R,N,3] and camera centres
        (host [R,3]) are given: sum_r basis_k(xyz - centre_r) * colorCot_r."""
        xyz, colorCotAll = self._t(xyz), self._t(colorCotAll)
        R, N = int(colorCotAll.shape[0]), int(xyz.shape[0])
        cc = np.ascontiguousarray(camCenters, np.float32).reshape(R, 3)
        g = out or dict(features_dc=self._empty(N, 1, 3), features_rest=self._empty(N, K - 1, 3))
        self._check(self.lib.gs_sh_grad_from_views(self.ctx, N, K, R, _p(xyz), _p(colorCotAll),
                                                   cc.ctypes.data_as(C.c_void_p), _p(g["features_dc"]),
                                                   _p(g["features_rest"])))
        return g

    # -- densify / prune kernels (GaussianTrainer.swift:317-427) and the gather of :858-893 -----------------------
    def setGradNormAccum(self, accum):
        """Fuse the densification statistic into the backward: the following renderBackward* calls add |grad xyz| to
        accum [N] (None = off).  The tensor must stay alive while set."""
        self._grad_norm_accum = accum
        self._check(self.lib.gs_set_grad_norm_accum(self.ctx, _p(accum)))

    def accumGradNorm(self, xyzGrad, accumIn=None, out=None):
        xyzGrad = self._t(xyzGrad)
        N = int(xyzGrad.shape[0])
        out = self._empty(N) if out is None else out
        self._check(self.lib.gs_accum_grad_norm(self.ctx, N, _p(xyzGrad), _p(None if accumIn is None else self._t(accumIn)),
                                                _p(out)))
        return out

    def classifyGaussians(self, gradAccum, denom: float, scales, opacity, gradThreshold=0.0002, maxScale=0.01,
                          minOpacity=0.005, allowDensify=True):
        gradAccum, scales, opacity = self._t(gradAccum), self._t(scales), self._t(opacity)
        N = int(gradAccum.shape[0])
        actions, counts = self._empty(N, dtype=torch.int32), self._empty(N, dtype=torch.int32)
        self._check(self.lib.gs_classify_gaussians(self.ctx, N, _p(gradAccum), C.c_float(denom), _p(scales),
                                                   int(scales.shape[1]) if N else 3, _p(opacity), C.c_float(gradThreshold),
                                                   C.c_float(maxScale), C.c_float(minOpacity), int(bool(allowDensify)),
                                                   _p(actions), _p(counts)))
        return actions, counts

    def densifyOffsets(self, actions, counts):
        """Exclusive scan of the output counts + action counts; synchronises (the reference's .item())."""
        N = int(actions.shape[0])
        offsets = self._empty(N, dtype=torch.int32)
        st = (C.c_longlong * 5)()
        self._check(self.lib.gs_densify_offsets(self.ctx, N, _p(actions), _p(counts), _p(offsets), st))
        return offsets, dict(zip(("total", "keep", "split", "clone", "prune"), (int(x) for x in st)))

    def buildDensifyOutputMap(self, actions, offsets, total: int):
        gather, mode = self._empty(total, dtype=torch.int32), self._empty(total, dtype=torch.int32)
        self._check(self.lib.gs_build_densify_output_map(self.ctx, int(actions.shape[0]), _p(actions), _p(offsets),
                                                         int(total), _p(gather), _p(mode)))
        return gather, mode

    # -- the planned event (gs_densify_plan ...): the count stays on the device, the host waits for the plan alone ----------
    def densifyPlan(self, actions, counts):
        """The scan of densifyOffsets without its wait; the plan stays in the context (densifyPlanRead)."""
        N = int(actions.shape[0])
        offsets = self._empty(N, dtype=torch.int32)
        self._check(self.lib.gs_densify_plan(self.ctx, N, _p(actions), _p(counts), _p(offsets)))
        return offsets

    def densifyPlanRead(self, wait: bool = True):
        """dict(N_new, applies, total, keep, split, clone, prune, N) once the plan kernel has run, else None (wait=False)."""
        plan, ready = (C.c_longlong * 8)(), C.c_int()
        self._check(self.lib.gs_densify_plan_read(self.ctx, int(bool(wait)), plan, C.byref(ready)))
        if not ready.value:
            return None
        return dict(zip(("N_new", "applies", "total", "keep", "split", "clone", "prune", "N"), (int(x) for x in plan)))

    def buildDensifyOutputMapPlanned(self, actions, offsets, capacity: int):
        gather, mode = self._empty(capacity, dtype=torch.int32), self._empty(capacity, dtype=torch.int32)
        self._check(self.lib.gs_build_densify_output_map_planned(self.ctx, int(actions.shape[0]), _p(actions), _p(offsets),
                                                                 int(capacity), _p(gather), _p(mode)))
        return gather, mode

    def densifyGatherPlanned(self, params: dict, gather, noiseMode, noiseSeed: int, out: dict, capacity: int):
        """out: views whose POINTERS are used (rows [0, new count) are written: the storage behind them must hold
        min(new count, capacity) rows)."""
        p = {k: self._t(v) for k, v in params.items()}
        K = int(p["features_rest"].shape[1]) + 1
        self._check(self.lib.gs_densify_gather_planned(self.ctx, int(capacity), K, _p(p["xyz"]), _p(p["features_dc"]),
                                                       _p(p["features_rest"]), _p(p["scales"]), _p(p["rotation"]),
                                                       _p(p["opacity"]), _p(gather), _p(noiseMode),
                                                       C.c_ulonglong(int(noiseSeed) & 0xFFFFFFFFFFFFFFFF), _p(out["xyz"]),
                                                       _p(out["features_dc"]), _p(out["features_rest"]), _p(out["scales"]),
                                                       _p(out["rotation"]), _p(out["opacity"])))

    # tensor ids of gs_densify_gather_planned_packed's arena_order (the reference's parameter order, GaussianModel.swift:46-55)
    _PACKED_IDS = dict(xyz=0, features_dc=1, features_rest=2, scales=3, rotation=4, opacity=5)

    def densifyGatherPlannedPacked(self, params: dict, gather, noiseMode, noiseSeed: int, outBase, capacity: int, arenaOrder):
        """The planned gather into a PACKED arena at outBase (a flat float tensor with room for `capacity` Gaussians): every
        tensor's segment is sized by the plan's new count, padded to four floats, in arenaOrder (tensor names in the order
        they lie in the arena); the tensor starts are computed on the device behind the plan (ABI 6)."""
        p = {k: self._t(v) for k, v in params.items()}
        K = int(p["features_rest"].shape[1]) + 1
        order = (C.c_int * 6)(*[self._PACKED_IDS[k] for k in arenaOrder])
        self._check(self.lib.gs_densify_gather_planned_packed(self.ctx, int(capacity), K, _p(p["xyz"]), _p(p["features_dc"]),
                                                              _p(p["features_rest"]), _p(p["scales"]), _p(p["rotation"]),
                                                              _p(p["opacity"]), _p(gather), _p(noiseMode),
                                                              C.c_ulonglong(int(noiseSeed) & 0xFFFFFFFFFFFFFFFF), _p(outBase), order))

    def densifyNoise(self, seed: int, rows: int):
        """[rows, 3] standard normal, row j a function of (seed, j) alone: what the planned gather adds, as a tensor."""
        out = self._empty(int(rows), 3)
        self._check(self.lib.gs_densify_noise(self.ctx, C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), int(rows), _p(out)))
        return out

    def densifyGather(self, params: dict, gather, noiseMode, baseNoise=None, out: dict | None = None):
        p = {k: self._t(v) for k, v in params.items()}
        total, K = int(gather.shape[0]), int(p["features_rest"].shape[1]) + 1
        o = out or {k: self._empty(total, *v.shape[1:]) for k, v in p.items()}
        nz = None if baseNoise is None else self._t(baseNoise)
        self._check(self.lib.gs_densify_gather(self.ctx, total, K, _p(p["xyz"]), _p(p["features_dc"]),
                                               _p(p["features_rest"]), _p(p["scales"]), _p(p["rotation"]),
                                               _p(p["opacity"]), _p(gather), _p(noiseMode), _p(nz), _p(o["xyz"]),
                                               _p(o["features_dc"]), _p(o["features_rest"]), _p(o["scales"]),
                                               _p(o["rotation"]), _p(o["opacity"])))
        return o

    # -- SSIM custom function + loss (GaussianTrainer.swift:555-723) --------------------------------------------
    def ssim(self, img1, img2, window=None, K: int = 11):
        img1, img2 = self._t(img1), self._t(img2)
        H, W, Cc = img1.shape
        window = self.ssimWindow if window is None else self._t(window)
        outs = [self._empty(H, W, Cc) for _ in range(6)]
        self._check(self.lib.gs_ssim_forward(self.ctx, H, W, Cc, K, _p(img1), _p(img2), _p(window),
                                             *[_p(o) for o in outs]))
        self._ssim_saved = (img1, img2, window, K, outs[1:])
        return outs

    def ssimVJP(self, gradOut, saved=None):
        img1, img2, window, K, maps = saved or self._ssim_saved
        H, W, Cc = img1.shape
        gradOut = self._t(gradOut)
        g1, g2 = torch.empty_like(img1), torch.empty_like(img2)
        self._check(self.lib.gs_ssim_backward(self.ctx, H, W, Cc, K, _p(gradOut), _p(img1), _p(img2), _p(window),
                                              *[_p(m) for m in maps], _p(g1), _p(g2)))
        return g1, g2

    def lossForwardBackward(self, render, target, lambda_dssim: float = 0.2, renderDepth=None, targetDepth=None,
                            depthMask=None, lambda_depth: float = 0.0, out=None, targetKey=None):
        """targetKey: any hashable naming the target image (e.g. the training view index).  When given, the target's
        windowed statistics are kept in a per-key device buffer at the first call (15 MB at 800x800) and read back at the
        later ones (gs_set_loss_target_cache); the results are bit-identical either way.  A key whose target tensor has
        changed (another storage, or written in place since), or that was filled under another loss mask (setLossMask: another
        tensor, none, or the same written in place since), is refilled; the caches together are capped at
        targetStatsCacheBytes, least recently used keys first."""
        render, target = self._t(render), self._t(target)
        ent = None
        if targetKey is not None and self.targetStatsCache:
            # an entry is valid for ONE image: same storage and no in-place write since it was filled (a target rewritten in
            # place, or another image in a reused allocator block, refills it); invalidateTarget(key) drops it explicitly
            # ... under ONE mask: the statistics are those of the weighted target (gs_set_loss_mask)
            lm = self._loss_mask
            ident = (target.data_ptr(), target._version, tuple(target.shape), None if lm is None else (lm.data_ptr(), lm._version))
            ent = self._target_cache.get(targetKey)
            if ent is None or ent[1] != ident:
                n = C.c_longlong()
                self._check(self.lib.gs_loss_target_cache_floats(self.ctx, C.byref(n)))
                ent = [self._empty(n.value) if ent is None else ent[0], ident, 0]
                self._target_cache[targetKey] = ent
                # the key being served is the most recently used one BEFORE anything is evicted: a refilled key kept its old
                # position, and with the cache over the cap (targetStatsCacheBytes lowered since) the loop below could pop that
                # very key and the step died in a KeyError (round 4's advisor)
                self._target_cache.move_to_end(targetKey)
                # byte cap: least recently used keys go first (tens of GB otherwise on large images with many views)
                while len(self._target_cache) > 1 and 4 * n.value * len(self._target_cache) > self.targetStatsCacheBytes:
                    self._target_cache.popitem(last=False)
            self._target_cache.move_to_end(targetKey)
            self._check(self.lib.gs_set_loss_target_cache(self.ctx, _p(ent[0]), ent[2]))
        else:
            self._check(self.lib.gs_set_loss_target_cache(self.ctx, None, 0))
        lossOut = out["loss"] if out else self._empty(4)
        cotColor = out["cotColor"] if out else torch.empty_like(render)
        cotDepth = None
        rd = td = dm = None
        if lambda_depth != 0.0:
            rd, td = self._t(renderDepth), self._t(targetDepth)
            dm = depthMask.to(device=self.device, dtype=torch.uint8).contiguous()
            cotDepth = self._empty(self.H, self.W)
        self._cuts_renewed()
        self._check(self.lib.gs_loss_forward_backward(self.ctx, _p(render), _p(target), _p(rd), _p(td), _p(dm),
                                                      C.c_float(lambda_dssim), C.c_float(lambda_depth), _p(lossOut),
                                                      _p(cotColor), _p(cotDepth)))
        if ent is not None:
            ent[2] = 1          # filled -- only now that the kernel which fills it has been queued without an error
        return lossOut, cotColor, cotDepth

    # -- depth supervision (include/gsplat.h gs_depth_loss; depth_loss.py) ------------------------------
    @staticmethod
    def depthLossParams(mode, weight: float, alpha_min: float = 0.05, scale: float = 1.0, offset: float = 0.0):
        """gs_depth_loss_params: mode by name (depth_loss.MODES) or number, the term's weight (the header's lambda), alpha_min,
        and the target's scale and offset (t = scale * target + offset)."""
        from .depth_loss import MODES
        if isinstance(mode, str):
            if mode not in MODES:
                raise ValueError(f"depthLossParams: unknown mode {mode!r} (one of {', '.join(MODES)})")
            mode = MODES.index(mode)
        return _lib.gs_depth_loss_params(int(mode), float(weight), float(alpha_min), float(scale), float(offset))

    def depthLoss(self, renderDepth, renderAlpha, target, mask, params, out=None):
        """gs_depth_loss on a render's depth and alpha images ([H, W] or [H, W, 1]): returns (loss, cotDepth, cotAlpha), the
        cotangents [H, W] as the fused backwards take them.  mask: uint8 or bool, tensor or array, non-zero = the pixel takes
        part, or None = all (the depth term's own mask: setLossMask's is not read).  params: depthLossParams(...) or a dict of
        its arguments.  out: dict(loss=, cotDepth=, cotAlpha=) of buffers to use; loss is the float[4] a lossForwardBackward
        has written -- loss[3] becomes the depth term and loss[0] gains weight times it -- and starts at zero without out.
        renderAlpha and cotAlpha may be None in the accumulated mode (the returned cotAlpha is then None)."""
        p = params if isinstance(params, _lib.gs_depth_loss_params) else self.depthLossParams(**params)
        P = self.H * self.W
        rd, tg = self._t(renderDepth), self._t(target)
        ra = None if renderAlpha is None else self._t(renderAlpha)
        if rd.numel() != P or tg.numel() != P or (ra is not None and ra.numel() != P):
            raise ValueError(f"depthLoss: render depth, render alpha and target are [H, W] = [{self.H}, {self.W}] images")
        dm = None
        if mask is not None:
            dm = mask if torch.is_tensor(mask) else torch.as_tensor(np.ascontiguousarray(mask))
            if dm.dtype not in (torch.uint8, torch.bool) or dm.numel() != P:
                raise ValueError(f"depthLoss: mask is a uint8 or bool [H, W] = [{self.H}, {self.W}] image, or None")
            dm = dm.to(device=self.device, dtype=torch.uint8).contiguous()
        out = out or {}
        loss = out["loss"] if "loss" in out else torch.zeros(4, device=self.device)
        cotDepth = out["cotDepth"] if "cotDepth" in out else self._empty(self.H, self.W)
        cotAlpha = out["cotAlpha"] if "cotAlpha" in out else (None if ra is None else self._empty(self.H, self.W))
        for name, t, n in (("loss", loss, 4), ("cotDepth", cotDepth, P), ("cotAlpha", cotAlpha, P)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device or t.numel() != n):
                raise ValueError(f"depthLoss: out[{name!r}] is a contiguous float32 device tensor of {n} elements")
        self._check(self.lib.gs_depth_loss(self.ctx, C.byref(p), _p(rd), _p(ra), _p(tg), _p(dm), _p(loss), _p(cotDepth),
                                           _p(cotAlpha)))
        return loss, cotDepth, cotAlpha

    def expectedDepth(self, res, alpha_min: float = 0.05):
        """gs_depth_normalize: the expected depth D / a of a render (a RenderResult with its depth image, or a (depth, alpha)
        pair) where a >= alpha_min and a > 0, 0 elsewhere; a new tensor of the depth image's shape."""
        depth, alpha = (res.depth, res.alpha) if hasattr(res, "depth") else res
        if depth is None:
            raise ValueError("expectedDepth: the render has no depth image (renderForward(wantDepth=True))")
        d, a = self._t(depth), self._t(alpha)
        if d.numel() != a.numel():
            raise ValueError("expectedDepth: depth and alpha are images of one size")
        out = torch.empty_like(d)
        self._check(self.lib.gs_depth_normalize(self.ctx, d.numel(), _p(d), _p(a), C.c_float(alpha_min), _p(out)))
        return out

    # -- normal regularisation (include/gsplat.h gs_normal_loss / gs_depth_normals; normal_loss.py) -------
    def _pinhole(self, camera, who):
        """(fx, fy, cx, cy) of a pinhole camera: a Camera, its as_dict(), a gs_camera (the principal point read back from its
        projection matrix's offsets, camera.py) or a sequence of the four; a fisheye one is refused."""
        if isinstance(camera, _lib.gs_camera):
            model = "pinhole"
            K = (camera.focal_x, camera.focal_y, (camera.proj[8] + 1.0) * self.W / 2.0, (camera.proj[9] + 1.0) * self.H / 2.0)
        elif isinstance(camera, dict):
            model = camera.get("model", "pinhole")
            K = (camera["focalX"], camera["focalY"], camera.get("principalX", self.W / 2.0), camera.get("principalY", self.H / 2.0))
        elif hasattr(camera, "focalX"):
            model = getattr(camera, "model", "pinhole")
            K = (camera.focalX, camera.focalY, getattr(camera, "principalX", self.W / 2.0), getattr(camera, "principalY", self.H / 2.0))
        else:
            model, K = "pinhole", tuple(camera)
            if len(K) != 4:
                raise ValueError(f"{who}: camera is a Camera, its as_dict() or (fx, fy, cx, cy)")
        if model != "pinhole":
            raise ValueError(f"{who}: a {model} camera is not served: the normals of a depth image are taken along pinhole rays "
                             "(rx, ry, 1); DESIGN.md section 34")
        return tuple(float(x) for x in K)

    def depthNormals(self, res, camera, alpha_min: float = 0.05, max_jump: float = 0.0):
        """gs_depth_normals: the normals of a render's expected depth image D / a in camera space (OpenCV axes, facing the
        camera), [H, W, 3]; the zero vector where a pixel has none -- the image's border, a pixel that is not depth-valid
        (a >= alpha_min, a > 0, D > 0) or has such a neighbour, and with max_jump > 0 a depth edge.  res: a RenderResult with
        its depth image, or a (depth, alpha) pair of [H, W] images of any one size.  A fisheye camera is refused."""
        depth, alpha = (res.depth, res.alpha) if hasattr(res, "depth") else res
        if depth is None:
            raise ValueError("depthNormals: the render has no depth image (renderForward(wantDepth=True))")
        K = self._pinhole(camera, "depthNormals")
        d, a = self._t(depth), self._t(alpha)
        if d.dim() == 3 and d.shape[-1] == 1:
            d, a = d.reshape(d.shape[:2]), a.reshape(d.shape[:2])
        if d.dim() != 2 or d.numel() != a.numel():
            raise ValueError("depthNormals: depth and alpha are [H, W] images of one size")
        H, W = int(d.shape[0]), int(d.shape[1])
        out = self._empty(H, W, 3)
        self._check(self.lib.gs_depth_normals(self.ctx, (C.c_float * 4)(*K), H, W, _p(d), _p(a), C.c_float(alpha_min),
                                              C.c_float(max_jump), _p(out)))
        return out

    def normalLossParams(self, camera, l1_weight: float = 0.0, cos_weight: float = 0.0, smooth_weight: float = 0.0,
                         alpha_min: float = 0.05, max_jump: float = 0.0, edge_gamma: float = 0.0, accumulate: bool = False):
        """gs_normal_loss_params for this renderer's H x W image under a pinhole camera (a Camera, its as_dict() or
        (fx, fy, cx, cy)): the three weights (the header's lambda_l1, lambda_cos, lambda_smooth), alpha_min, max_jump,
        edge_gamma and whether the cotangents are added to what the buffers hold."""
        K = self._pinhole(camera, "normalLossParams")
        return _lib.gs_normal_loss_params(*K, self.H, self.W, float(l1_weight), float(cos_weight), float(smooth_weight),
                                          float(alpha_min), float(max_jump), float(edge_gamma), int(bool(accumulate)))

    def normalLoss(self, renderDepth, renderAlpha, camera, targetNormal, mask, edgeImage, params, out=None):
        """gs_normal_loss on a render's depth and alpha images ([H, W] or [H, W, 1]): returns (loss, terms, cotDepth, cotAlpha),
        terms = (L_l1, L_cos, L_s) on the device and the cotangents [H, W] as the fused backwards take them.  targetNormal:
        [H, W, 3] in camera space, OpenCV axes, facing the camera (normalised by the kernel; squared norm < 0.25 is a hole), or
        None: the smoothness term alone.  mask: uint8 or bool, non-zero = the pixel takes part in the prior terms, or None = all.
        edgeImage: [H, W, 3] or None.  params: normalLossParams(camera, ...) or a dict of its keyword arguments; the camera's
        intrinsics are taken from `camera` either way.  out: dict(loss=, terms=, cotDepth=, cotAlpha=) of buffers to use; loss is
        the float[4] a lossForwardBackward has written -- loss[0] gains the weighted terms -- and starts at zero without out; with
        params.accumulate the cotangents are added to what out's buffers hold (a depthLoss queued before)."""
        if isinstance(params, _lib.gs_normal_loss_params):
            K = self._pinhole(camera, "normalLoss")
            p = _lib.gs_normal_loss_params(*K, self.H, self.W, params.lambda_l1, params.lambda_cos, params.lambda_smooth,
                                           params.alpha_min, params.max_jump, params.edge_gamma, params.accumulate)
        else:
            p = self.normalLossParams(camera, **params)
        P = self.H * self.W
        rd, ra = self._t(renderDepth), self._t(renderAlpha)
        if rd.numel() != P or ra.numel() != P:
            raise ValueError(f"normalLoss: render depth and render alpha are [H, W] = [{self.H}, {self.W}] images")
        tn = None if targetNormal is None else self._t(targetNormal)
        ei = None if edgeImage is None else self._t(edgeImage)
        for name, t in (("targetNormal", tn), ("edgeImage", ei)):
            if t is not None and t.numel() != 3 * P:
                raise ValueError(f"normalLoss: {name} is [H, W, 3] = [{self.H}, {self.W}, 3], or None")
        nm = None
        if mask is not None:
            nm = mask if torch.is_tensor(mask) else torch.as_tensor(np.ascontiguousarray(mask))
            if nm.dtype not in (torch.uint8, torch.bool) or nm.numel() != P:
                raise ValueError(f"normalLoss: mask is a uint8 or bool [H, W] = [{self.H}, {self.W}] image, or None")
            nm = nm.to(device=self.device, dtype=torch.uint8).contiguous()
        out = out or {}
        if p.accumulate and not ("cotDepth" in out and "cotAlpha" in out):
            raise ValueError("normalLoss: accumulate adds to out['cotDepth'] and out['cotAlpha']: pass both")
        loss = out["loss"] if "loss" in out else torch.zeros(4, device=self.device)
        terms = out["terms"] if "terms" in out else self._empty(3)
        cotDepth = out["cotDepth"] if "cotDepth" in out else self._empty(self.H, self.W)
        cotAlpha = out["cotAlpha"] if "cotAlpha" in out else self._empty(self.H, self.W)
        for name, t, n in (("loss", loss, 4), ("terms", terms, 3), ("cotDepth", cotDepth, P), ("cotAlpha", cotAlpha, P)):
            if t is None or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device or t.numel() != n:
                raise ValueError(f"normalLoss: out[{name!r}] is a contiguous float32 device tensor of {n} elements")
        self._check(self.lib.gs_normal_loss(self.ctx, C.byref(p), _p(rd), _p(ra), _p(tn), _p(nm), _p(ei), _p(loss), _p(terms),
                                            _p(cotDepth), _p(cotAlpha)))
        return loss, terms, cotDepth, cotAlpha

    # -- held-out evaluation (include/gsplat.h gs_image_metrics / gs_colour_moments; evaluation.py) ------
    def _metric_mask(self, who, mask, H, W):
        """A uint8 or bool [H, W] mask, tensor or array, as the contiguous uint8 device tensor the kernels read (itself if it is one)."""
        loss_mask.validate(mask, H, W, who)
        if not torch.is_tensor(mask):
            mask = torch.from_numpy(np.ascontiguousarray(loss_mask.as_uint8(mask)))
        if mask.dtype == torch.bool:
            mask = mask.to(torch.uint8) * 255
        return mask.to(self.device).contiguous()

    def _metric_args(self, who, render, target, mask, out, n_out):
        render, target = self._t(render), self._t(target)
        if render.dim() != 3 or render.shape[-1] != 3 or render.shape != target.shape:
            raise ValueError(f"{who}: render and target are [H, W, 3] images of one size")
        H, W = int(render.shape[0]), int(render.shape[1])
        if mask is not None:
            mask = self._metric_mask(who, mask, H, W)
        if out is None:
            out = torch.empty(n_out, dtype=torch.float64, device=self.device)
        elif out.dtype != torch.float64 or not out.is_contiguous() or out.device != self.device or out.numel() != n_out:
            raise ValueError(f"{who}: out is a contiguous float64 device tensor of {n_out} elements")
        return render, target, mask, out, H, W

    def imageMetrics(self, render, target, mask=None, out=None):
        """gs_image_metrics: {sse, ssim_sum, wsum, 3 wsum} of a render against its target, both [H, W, 3] of any one size and
        clamped to [0, 1] by the kernel -- a device float64 tensor [4] (evaluation.metrics_from_sums turns it into PSNR and
        SSIM).  mask: uint8 (weight v / 255) or bool [H, W], tensor or array, or None.  out: a float64 device tensor of 4
        elements to write into (a row of a [V, 4] buffer).  Does not wait."""
        render, target, mask, out, H, W = self._metric_args("imageMetrics", render, target, mask, out, 4)
        self._check(self.lib.gs_image_metrics(self.ctx, H, W, _p(render), _p(target), _p(mask), _p(out)))
        return out

    def colourMoments(self, render, target, mask=None, out=None):
        """gs_colour_moments: the 22 moment sums of the affine colour fit of render onto target (evaluation.fit_affine_colour
        solves them for M) -- a device float64 tensor [22].  Arguments as imageMetrics'.  Does not wait."""
        render, target, mask, out, H, W = self._metric_args("colourMoments", render, target, mask, out, 22)
        self._check(self.lib.gs_colour_moments(self.ctx, H * W, _p(render), _p(target), _p(mask), _p(out)))
        return out

    def invalidateTarget(self, targetKey=None):
        """Forget the cached SSIM statistics of one target key (None: of all): its next loss recomputes them."""
        if targetKey is None:
            self._target_cache.clear()
        else:
            self._target_cache.pop(targetKey, None)
