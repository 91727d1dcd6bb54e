"""Host-side mirror of the reference's dataset loaders (Data/ColmapDataLoader.swift, Data/NerfStudioDataLoader.swift,
Data/BlenderDataLoader.swift): file formats, pose / intrinsics conventions, the TrainData container.

What is mirrored exactly: the binary / JSON / PLY parsing, quaternion -> rotation, world-to-camera inversion, the
OpenGL -> OpenCV flip (rows 1-2 of w2c negated), intrinsics scaling by resizeFactor, white-background compositing,
the tile size rule (W/4, H/4).  Not in the reference: per-view loss masks (readMask, TrainData.maskArray)
and COLMAP sets with Inria's inverse-depth priors (readInverseDepth, TrainData.depthArray / depthAlign);
COLMAP's own camera-model table and lens undistortion at load time (cameraModels="colmap", undistort=True).
What is not mirrored: image decoding and resampling (the reference goes through UIKit /
CoreGraphics; here PIL, bilinear) and the downloads / unzipping of the demo sets (no network: loaders take paths)."""
from __future__ import annotations

import json
import os
import struct
from collections import namedtuple
import dataclasses
from dataclasses import dataclass

import numpy as np

from .pointcloud import PointCloud, getPointCloudsFromTrainData

TILE_SIZE_H_W = namedtuple("TILE_SIZE_H_W", ["w", "h"])


@dataclass
class TrainData:
    Hs: np.ndarray
    Ws: np.ndarray
    intrinsicArray: np.ndarray
    c2wArray: np.ndarray
    rgbArray: np.ndarray
    alphaArray: np.ndarray
    depthArray: np.ndarray | None = None
    maskArray: np.ndarray | None = None       # uint8 [n, H, W] loss masks (255 keeps a pixel), None when no view has one
    depthAlign: np.ndarray | None = None      # float32 [n, 2]: (scale, offset) to apply to depthArray's view (trainStep's depthAlign)
    # str [n]: "pinhole" or "fisheye" per view (camera.Camera's model), None: all pinhole.  Set by the loaders' fisheye="equidistant"
    # after construction -- an attribute, not a dataclass field: code that walks dataclasses.fields(TrainData) takes every field for
    # a per-view array that is there.  copy.copy / copy.deepcopy keep it; dataclasses.replace() builds a new object from the fields
    # alone and would drop it -- a fisheye view would then train as a pinhole with a fisheye's focal length: use replace() below.
    cameraModelArray = None
    # float32 [n, H, W, 3]: per-view normal priors in camera space, OpenCV axes, facing the camera (trainStep's targetNormal;
    # DESIGN.md section 34); a hole is the zero vector.  None: no view has one.  Set by the loaders' normalRoot= after
    # construction -- an attribute beside the fields, for cameraModelArray's reason, and carried by replace() as it is.
    normalArray = None

    def getCameraParams(self):
        return self.Hs, self.Ws, self.intrinsicArray, self.c2wArray

    def replace(self, **changes):
        """dataclasses.replace that keeps cameraModelArray and normalArray (or takes new ones: replace(cameraModelArray=...))."""
        models = changes.pop("cameraModelArray", self.cameraModelArray)
        normals = changes.pop("normalArray", self.normalArray)
        out = dataclasses.replace(self, **changes)
        out.cameraModelArray = models
        out.normalArray = normals
        return out


# ---- images ---------------------------------------------------------------------------------------------------
def _load_image(path, scale: float, mode: str):
    from PIL import Image
    img = Image.open(path).convert(mode)
    if scale != 1.0:
        img = img.resize((int(img.size[0] * scale), int(img.size[1] * scale)), Image.BILINEAR)
    return np.asarray(img, np.float32) / np.float32(255.0)


def readImageRGBA(path, resizeFactor: float = 1.0):
    """ColmapDataLoader.readImage / NerfStudio readImage: rgb [H,W,3], alpha [H,W], H, W (floats in [0,1])."""
    rgba = _load_image(path, resizeFactor, "RGBA")
    return rgba[..., :3], rgba[..., 3], float(rgba.shape[0]), float(rgba.shape[1])


def readMask(path, resizeFactor: float = 1.0):
    """A view's loss mask (trainStep's lossMask): uint8 [H, W], the file's grey levels (PIL mode "L") under the images' own
    bilinear resize.  White keeps a pixel; nothing is inverted or thresholded."""
    from PIL import Image
    img = Image.open(path).convert("L")
    if resizeFactor != 1.0:
        img = img.resize((int(img.size[0] * resizeFactor), int(img.size[1] * resizeFactor)), Image.BILINEAR)
    return np.array(img, np.uint8)


def readInverseDepth(path, resizeFactor: float = 1.0):
    """A view's depth prior in Inria's layout: a 16-bit PNG whose value / 65536 is the inverse depth, float32 [H, W], under the
    images' own bilinear resize (taken on the float values).  0 is a hole."""
    from PIL import Image
    raw = np.array(Image.open(path))
    if raw.ndim != 2 or raw.dtype.kind not in "ui":
        raise ValueError(f"depth map {path}: a single-channel integer PNG (16-bit) is expected")
    inv = raw.astype(np.float32) / np.float32(65536.0)
    if resizeFactor != 1.0:
        img = Image.fromarray(inv)          # (float32: mode "F")
        img = img.resize((int(img.size[0] * resizeFactor), int(img.size[1] * resizeFactor)), Image.BILINEAR)
        inv = np.array(img, np.float32)
    return inv


NORMAL_CONVENTIONS = ("opencv", "opengl")


def readNormalMap(path, resizeFactor: float = 1.0, convention: str = "opencv"):
    """A view's normal prior (trainStep's targetNormal): an 8- or 16-bit RGB PNG whose value v in [0, 1] is the component
    2 v - 1, float32 [H, W, 3] in camera space, under the images' own bilinear resize (taken on the float components; the
    kernel normalises).  Eight bits of precision either way: PIL has no 16-bit RGB image and hands on a 16-bit file's high
    bytes, so a component of such a file is up to 2 / 255 off -- under a degree, below any monocular estimator's own error.
    convention: "opencv" (x right, y down, z forward: a surface facing the camera has z < 0) takes the file as it is;
    "opengl" (x right, y up, z backward, what most monocular estimators write) flips y and z."""
    from PIL import Image
    if convention not in NORMAL_CONVENTIONS:
        raise ValueError(f'normalConvention is one of {", ".join(NORMAL_CONVENTIONS)}')
    raw = np.array(Image.open(path))
    if raw.ndim != 3 or raw.shape[2] < 3 or raw.dtype != np.uint8:      # (what PIL makes of an RGB or RGBA file of either depth)
        raise ValueError(f"normal map {path}: an 8- or 16-bit RGB PNG is expected")
    n = np.float32(2.0) * (raw[..., :3].astype(np.float32) / np.float32(255.0)) - np.float32(1.0)
    if resizeFactor != 1.0:
        size = (int(raw.shape[1] * resizeFactor), int(raw.shape[0] * resizeFactor))
        n = np.stack([np.array(Image.fromarray(np.ascontiguousarray(n[..., c])).resize(size, Image.BILINEAR), np.float32)
                      for c in range(3)], -1)
    if convention == "opengl":
        n = n * np.array([1.0, -1.0, -1.0], np.float32)
    return np.ascontiguousarray(n, np.float32)


def _check_normals(normalRoot, normalConvention, undistort, who):
    if normalConvention not in NORMAL_CONVENTIONS:
        raise ValueError(f'{who}: normalConvention is one of {", ".join(NORMAL_CONVENTIONS)}')
    if normalRoot is not None and undistort:
        raise ValueError(f"{who}: normalRoot does not go with undistort=True (resampling a view bends its rays: its normal prior "
                         "would have to be resampled and its directions rotated, which is not done here)")


def _stack_normals(paths, Hs, Ws, resizeFactor: float, convention: str):
    """normalArray of the views whose normal maps are `paths` (None or a missing file: the view is all holes)."""
    out = []
    for p, H, W in zip(paths, Hs, Ws):
        n = readNormalMap(p, resizeFactor, convention) if p is not None and os.path.exists(p) else np.zeros((int(H), int(W), 3), np.float32)
        if n.shape != (int(H), int(W), 3):
            raise ValueError(f"normal map {p}: {n.shape[1]} x {n.shape[0]} after the resize, its image is {int(W)} x {int(H)}")
        out.append(n)
    return np.stack(out).astype(np.float32)


def readDepthParams(depthParams) -> dict:
    """Inria's depth_params.json -- {image stem: {"scale": s, "offset": o, ...}} -- as a dict, from a dict or a path to the file."""
    if depthParams is None:
        return {}
    if isinstance(depthParams, (str, os.PathLike)):
        with open(depthParams) as f:
            depthParams = json.load(f)
    if not isinstance(depthParams, dict):
        raise ValueError("depthParams is the depth_params.json dict or a path to it")
    return depthParams


def _stack_masks(paths, Hs, Ws, resizeFactor: float):
    """maskArray of the views whose mask files are `paths` (None: the view has none): None when no view has a mask, else
    uint8 [n, H, W] with all 255 (keep everything) for a view without one."""
    if all(p is None for p in paths):
        return None
    masks = []
    for p, H, W in zip(paths, Hs, Ws):
        m = np.full((int(H), int(W)), 255, np.uint8) if p is None else readMask(p, resizeFactor)
        if m.shape != (int(H), int(W)):
            raise ValueError(f"mask {p}: {m.shape[1]} x {m.shape[0]} after the resize, its image is {int(W)} x {int(H)}")
        masks.append(m)
    return np.stack(masks)


def _stack_frames(frames, whiteBackground: bool):
    rgbs = np.stack([f[0] for f in frames]); alphas = np.stack([f[1] for f in frames])
    if whiteBackground:
        rgbs = alphas[..., None] * rgbs + (1 - alphas)[..., None]
    Hs = np.array([f[2] for f in frames], np.float32); Ws = np.array([f[3] for f in frames], np.float32)
    return Hs, Ws, rgbs.astype(np.float32), alphas.astype(np.float32)


# ---- lens undistortion (lens.py; not in the reference) ---------------------------------------------------
def _host(x):
    """A numpy array of what an undistorter returned (lens.undistort_image: numpy; GaussianRenderer.undistortImage: tensors)."""
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _undistort_views(lenses, frames, masks, depths, undistorter=None):
    """The loaders' undistort=True pass, after the resize: every view i whose lenses[i] (a lens.LensModel with the view's
    SCALED K; None or a pinhole: the view is not resampled at all) has a non-zero coefficient is remapped into the pinhole
    with the same K -- RGBA in one colour call with four channels, the mask in mask mode, the depth prior in depth mode -- and
    its validity image is folded into the mask as an elementwise min.  frames: [(rgb, alpha, H, W)]; masks: uint8 [n, H, W]
    or None (created, all 255, when a view is resampled); depths: float32 [n, H, W] or None.  Returns (frames, masks, depths).
    undistorter(img, lens, mode=) -> (out, valid): lens.undistort_image by default (no GPU needed), or a renderer's
    undistortImage (the kernel)."""
    if undistorter is None:
        from .lens import undistort_image as undistorter
    # (a lens.FisheyeLensModel goes into the ideal equidistant camera with the same K: the loaders' fisheye="equidistant")
    todo = [i for i, L in enumerate(lenses) if L is not None and not getattr(L, "is_equidistant", getattr(L, "is_pinhole", False))]
    if not todo:
        return frames, masks, depths
    frames = list(frames)
    if masks is None:
        masks = np.stack([np.full((int(f[2]), int(f[3])), 255, np.uint8) for f in frames])
    else:
        masks = np.array(masks, np.uint8, copy=True)
    if depths is not None:
        depths = np.array(depths, np.float32, copy=True)
    for i in todo:
        rgb, alpha, H, W = frames[i]
        rgba = np.ascontiguousarray(np.concatenate([rgb, alpha[..., None]], axis=-1), np.float32)
        out, valid = undistorter(rgba, lenses[i], mode="color")
        out, valid = _host(out), _host(valid)
        frames[i] = (out[..., :3], out[..., 3], H, W)
        if not (masks[i] == 255).all():
            masks[i] = _host(undistorter(masks[i], lenses[i], mode="mask")[0])
        masks[i] = np.minimum(masks[i], valid)
        if depths is not None:
            depths[i] = _host(undistorter(depths[i], lenses[i], mode="depth")[0])
    return frames, masks, depths


# ---- COLMAP (ColmapDataLoader.swift:165-500) ---------------------------------------------------------------------
ColmapCamera = namedtuple("ColmapCamera", "id width height fx fy cx cy k1 k2 p1 p2 model", defaults=(None,))
ImageWithPose = namedtuple("ImageWithPose", "filePath pose cameraId")

# COLMAP's own camera models (src/colmap/sensor/models.h): id -> (name, number of doubles in cameras.bin)
COLMAP_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
# the models lens.LensModel inverts (k1, k2, p1, p2); the others load as pinholes and raise under undistort=True
UNDISTORTABLE = {"SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", None}
# the models lens.FisheyeLensModel resamples into the ideal equidistant camera under fisheye="equidistant" (DESIGN.md section 29):
# name -> where k1 .. k4 stand in the model's parameters (the missing ones are 0)
FISHEYE_MODELS = {"OPENCV_FISHEYE": (4, 4), "SIMPLE_RADIAL_FISHEYE": (3, 1), "RADIAL_FISHEYE": (3, 2)}


def _check_fisheye(fisheye, undistort, who):
    if fisheye not in (None, "equidistant"):
        raise ValueError(f'{who}: fisheye is None or "equidistant"')
    if fisheye is not None and not undistort:
        raise ValueError(f'{who}: fisheye="equidistant" goes with undistort=True (the views are resampled into the ideal camera)')


def colmapReadFisheyeCoefficients(binRoot):
    """{camera id: (k1, k2, k3, k4)} of the cameras.bin cameras whose model (COLMAP's own table) is one of FISHEYE_MODELS."""
    out = {}
    with open(os.path.join(binRoot, "cameras.bin"), "rb") as f:
        rd = lambda fmt: struct.unpack("<" + fmt, f.read(struct.calcsize("<" + fmt)))
        (n,) = rd("Q")
        for _ in range(n):
            camId, model = rd("Ii")
            rd("QQ")
            if model not in COLMAP_MODELS:
                raise ValueError(f"cameras.bin: camera {camId} has the unknown model id {model}")
            name, count = COLMAP_MODELS[model]
            p = rd("d" * count)
            if name in FISHEYE_MODELS:
                first, nk = FISHEYE_MODELS[name]
                out[camId] = tuple(p[first:first + nk]) + (0.0,) * (4 - nk)
    return out


def _colmapCamera(camId, model, width, height, p):
    """A COLMAP model's parameters (its own table) as a ColmapCamera: models 0-4 fill it; 5-10 keep their focal lengths and
    principal point (single-focal models: f, cx, cy) and no coefficients."""
    name = COLMAP_MODELS[model][0]
    k1 = k2 = p1 = p2 = None
    if name in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE"):
        fx, cx, cy = p[:3]; fy = fx
        if name == "SIMPLE_RADIAL":
            k1 = p[3]
        elif name == "RADIAL":
            k1, k2 = p[3:5]
    else:
        fx, fy, cx, cy = p[:4]
        if name == "OPENCV":
            k1, k2, p1, p2 = p[4:8]
    return ColmapCamera(camId, width, height, fx, fy, cx, cy, k1, k2, p1, p2, name)


def quatToRotMat(q):
    """:55-58: qvec = (w, x, y, z) -> 3x3 rotation (simd_quatd(ix: q1, iy: q2, iz: q3, r: q0))."""
    w, x, y, z = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def _intrinsics3(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def colmapReadCamerasAndPoses(binRoot, imageRoot, cameraModels: str = "reference"):
    """cameras.bin + images.bin -> ({camera id: ColmapCamera}, [ImageWithPose]); pose = camera-to-world
    [R^T | -R^T t] of the stored world-to-camera (qvec, tvec) (:258-296).  cameraModels="reference" is the reference app's
    model table (id 3 is OPENCV with 8 doubles, unknown models parse as PINHOLE, :199); "colmap" is COLMAP's own
    (COLMAP_MODELS: id 3 is RADIAL with 5 doubles, id 4 OPENCV with 8), every model read with its own count so that the file
    stays in step, and an unknown id raises."""
    if cameraModels not in ("reference", "colmap"):
        raise ValueError('cameraModels is "reference" or "colmap"')
    cam_path, img_path = os.path.join(binRoot, "cameras.bin"), os.path.join(binRoot, "images.bin")
    if not (os.path.exists(cam_path) and os.path.exists(img_path)):
        raise FileNotFoundError("Colmap files missing")
    camMap = {}
    with open(cam_path, "rb") as f:
        rd = lambda fmt: struct.unpack("<" + fmt, f.read(struct.calcsize("<" + fmt)))
        (n,) = rd("Q")
        for _ in range(n):
            camId, model = rd("Ii")
            width, height = rd("QQ")
            if cameraModels == "colmap":
                if model not in COLMAP_MODELS:
                    raise ValueError(f"cameras.bin: camera {camId} has the unknown model id {model}")
                camMap[camId] = _colmapCamera(camId, model, width, height, rd("d" * COLMAP_MODELS[model][1]))
                continue
            k1 = k2 = p1 = p2 = None
            name = "PINHOLE"
            if model == 0:                      # SIMPLE_PINHOLE
                fx, cx, cy = rd("ddd"); fy = fx; name = "SIMPLE_PINHOLE"
            elif model == 2:                    # SIMPLE_RADIAL
                fx, cx, cy, k1 = rd("dddd"); fy = fx; name = "SIMPLE_RADIAL"
            elif model == 3:                    # OPENCV
                fx, fy, cx, cy, k1, k2, p1, p2 = rd("dddddddd"); name = "OPENCV"
            else:                               # PINHOLE, and anything unknown
                fx, fy, cx, cy = rd("dddd")
            camMap[camId] = ColmapCamera(camId, width, height, fx, fy, cx, cy, k1, k2, p1, p2, name)
    poses = []
    with open(img_path, "rb") as f:
        rd = lambda fmt: struct.unpack("<" + fmt, f.read(struct.calcsize("<" + fmt)))
        (n,) = rd("Q")
        for _ in range(n):
            rd("I")                                              # image id
            q = rd("dddd"); t = np.array(rd("ddd"), np.float64)
            Rinv = quatToRotMat(q).T
            (camId,) = rd("I")
            name = bytearray()
            while True:
                ch = f.read(1)
                if not ch or ch == b"\x00":
                    break
                name += ch
            pose = np.eye(4, dtype=np.float64)
            pose[:3, :3] = Rinv
            pose[:3, 3] = -(Rinv @ t)
            (np2d,) = rd("Q")
            f.seek(24 * np2d, os.SEEK_CUR)                       # x, y (f64), point3D id (u64)
            poses.append(ImageWithPose(os.path.join(imageRoot, name.decode("utf-8")), pose, camId))
    return camMap, poses


def colmapReadPointSet(points3DPath):
    """points3D.bin -> (points [N,3] f64, colors [N,3] u8) (:398-440)."""
    pts, cols = [], []
    with open(points3DPath, "rb") as f:
        (n,) = struct.unpack("<Q", f.read(8))
        for _ in range(n):
            rec = f.read(8 + 24 + 3 + 8 + 8)
            _, x, y, z, r, g, b, _err, track = struct.unpack("<QdddBBBdQ", rec)
            pts.append((x, y, z)); cols.append((r, g, b))
            f.seek(8 * track, os.SEEK_CUR)
    return np.array(pts, np.float64).reshape(-1, 3), np.array(cols, np.uint8).reshape(-1, 3)


class ColmapDataLoader:
    def __init__(self, binRoot, imageRoot, maskRoot=None, depthRoot=None, depthParams=None, cameraModels: str = "reference",
                 undistort: bool = False, fisheye=None, normalRoot=None, normalConvention: str = "opencv"):
        """cameraModels: "reference" reads cameras.bin with the reference app's model table, "colmap" with COLMAP's own
        (colmapReadCamerasAndPoses); a real COLMAP reconstruction needs "colmap".

        undistort: resample every view whose camera has a non-zero lens coefficient (k1, k2, p1, p2) into its pinhole camera at
        load time (_undistort_views; the principal point is kept, camera.cameras_from_train_data renders it) and fold the
        validity of the resampling into TrainData.maskArray, so that the border the lens leaves empty is ignored by the loss.
        A camera model the lens module does not invert (fisheye, FULL_OPENCV, FOV) raises a ValueError in load().

        fisheye: None (the default: everything above, the ValueError for a fisheye camera included) or "equidistant", with
        cameraModels="colmap" and undistort=True: a view whose camera is OPENCV_FISHEYE, SIMPLE_RADIAL_FISHEYE or RADIAL_FISHEYE
        is resampled into the ideal equidistant camera with the same K (lens.FisheyeLensModel; validity folded into maskArray
        as above) and marked "fisheye" in TrainData.cameraModelArray, so that camera.cameras_from_train_data hands the trainer
        a Camera(model="fisheye").  THIN_PRISM_FISHEYE, FOV and FULL_OPENCV still raise.

        maskRoot: a directory of per-view loss masks (TrainData.maskArray).  A view's mask is <maskRoot>/<image file
        name>.png (COLMAP's own convention: "frame.jpg.png") or, failing that, <maskRoot>/<image file name without its
        extension>.png; a view with neither keeps every pixel.

        depthRoot: a directory of per-view depth priors in Inria's layout, <depthRoot>/<image stem>.png, 16-bit, value / 65536
        the inverse depth (TrainData.depthArray, the target of DepthConfig(mode="disparity")); a view without a file gets
        zeros, which the depth term's default mask (target > 0) leaves out.  depthParams: Inria's depth_params.json (the dict
        or a path to it): a view's "scale" and "offset" go to TrainData.depthAlign, (1, 0) for a view without an entry.

        normalRoot: a directory of per-view normal priors, <normalRoot>/<image stem>.png (readNormalMap: an 8- or 16-bit RGB
        PNG, v -> 2 v - 1, in normalConvention's axes), into TrainData.normalArray (trainStep's targetNormal; DESIGN.md section
        34); a view without a file is all holes.  Not with undistort=True."""
        self.binRoot, self.imageRoot, self.maskRoot = binRoot, imageRoot, maskRoot
        self.normalRoot, self.normalConvention = normalRoot, normalConvention
        _check_normals(normalRoot, normalConvention, undistort, "ColmapDataLoader")
        self.depthRoot, self.depthParams = depthRoot, readDepthParams(depthParams)
        self.cameraModels, self.undistort, self.fisheye = cameraModels, bool(undistort), fisheye
        if cameraModels not in ("reference", "colmap"):
            raise ValueError('cameraModels is "reference" or "colmap"')
        _check_fisheye(fisheye, undistort, "ColmapDataLoader")
        if fisheye is not None and cameraModels != "colmap":
            raise ValueError('ColmapDataLoader: fisheye="equidistant" goes with cameraModels="colmap" (the reference table has no fisheye model)')
        if depthRoot is None and depthParams is not None:
            raise ValueError("depthParams go with a depthRoot")

    def _depths(self, poses, Hs, Ws, resizeFactor: float):
        """(depthArray [n, H, W], depthAlign [n, 2]) of the views."""
        depths, align = [], []
        for p, H, W in zip(poses, Hs, Ws):
            stem = os.path.splitext(os.path.relpath(p.filePath, self.imageRoot))[0]
            path = os.path.join(self.depthRoot, stem + ".png")
            d = readInverseDepth(path, resizeFactor) if os.path.exists(path) else np.zeros((int(H), int(W)), np.float32)
            if d.shape != (int(H), int(W)):
                raise ValueError(f"depth map {path}: {d.shape[1]} x {d.shape[0]} after the resize, its image is {int(W)} x {int(H)}")
            depths.append(d)
            e = self.depthParams.get(stem, self.depthParams.get(os.path.basename(stem), {}))
            align.append((float(e.get("scale", 1.0)), float(e.get("offset", 0.0))))
        return np.stack(depths).astype(np.float32), np.asarray(align, np.float32).reshape(-1, 2)

    def _maskPath(self, imagePath):
        name = os.path.relpath(imagePath, self.imageRoot)
        for cand in (name + ".png", os.path.splitext(name)[0] + ".png"):
            if os.path.exists(os.path.join(self.maskRoot, cand)):
                return os.path.join(self.maskRoot, cand)
        return None

    def getOriginalImageSize(self):
        camMap, poses = colmapReadCamerasAndPoses(self.binRoot, self.imageRoot, self.cameraModels)
        cam = camMap[poses[0].cameraId]
        return int(cam.width), int(cam.height)

    def load(self, resizeFactor: float = 1.0, whiteBackground: bool = False, readImage=readImageRGBA, undistorter=None):
        """loadTrainDataAndPointCloud (:441-500) -> (TrainData, PointCloud, TILE_SIZE_H_W).  undistorter: what resamples a view
        under undistort=True (_undistort_views): None is lens.undistort_image on the host, a GaussianRenderer's undistortImage
        is the kernel."""
        camMap, poses = colmapReadCamerasAndPoses(self.binRoot, self.imageRoot, self.cameraModels)
        intr = np.stack([_intrinsics3(*(camMap[p.cameraId][3:7])) for p in poses])
        if resizeFactor != 1.0:
            intr[:, :2, :3] *= np.float32(resizeFactor)
        c2ws = np.stack([p.pose.astype(np.float32) for p in poses])
        frames = [readImage(p.filePath, resizeFactor) for p in poses]
        Hs, Ws = [f[2] for f in frames], [f[3] for f in frames]
        masks = None if self.maskRoot is None else _stack_masks([self._maskPath(p.filePath) for p in poses], Hs, Ws, resizeFactor)
        depths, align = (None, None) if self.depthRoot is None else self._depths(poses, Hs, Ws, resizeFactor)
        models = None
        if self.undistort:
            from .lens import FisheyeLensModel, LensModel
            lenses = []
            fish = colmapReadFisheyeCoefficients(self.binRoot) if self.fisheye == "equidistant" else {}
            if fish:
                models = np.array(["fisheye" if p.cameraId in fish else "pinhole" for p in poses])
            for p, K in zip(poses, intr):
                cam = camMap[p.cameraId]
                if p.cameraId in fish:
                    lenses.append(FisheyeLensModel(K[0, 0], K[1, 1], K[0, 2], K[1, 2], *fish[p.cameraId]))
                    continue
                if cam.model not in UNDISTORTABLE:
                    raise ValueError(f"undistort=True: camera {cam.id} has the model {cam.model}, which is not inverted here "
                                     "(SIMPLE_RADIAL, RADIAL and OPENCV are)")
                lenses.append(LensModel(K[0, 0], K[1, 1], K[0, 2], K[1, 2], cam.k1, cam.k2, cam.p1, cam.p2))
            frames, masks, depths = _undistort_views(lenses, frames, masks, depths, undistorter)
        Hs, Ws, rgbs, alphas = _stack_frames(frames, whiteBackground)
        pts, cols = colmapReadPointSet(os.path.join(self.binRoot, "points3D.bin"))
        ch = cols.astype(np.float32) / np.float32(255.0)
        pcd = PointCloud(pts.astype(np.float32), dict(R=ch[:, 0], G=ch[:, 1], B=ch[:, 2]))
        td = TrainData(Hs, Ws, intr, c2ws, rgbs, alphas, depths, masks, align)
        td.cameraModelArray = models
        if self.normalRoot is not None:
            stems = [os.path.splitext(os.path.relpath(p.filePath, self.imageRoot))[0] for p in poses]
            td.normalArray = _stack_normals([os.path.join(self.normalRoot, s + ".png") for s in stems], Hs, Ws, resizeFactor,
                                            self.normalConvention)
        return td, pcd, TILE_SIZE_H_W(w=int(Ws[0]) // 4, h=int(Hs[0]) // 4)


# ---- OpenGL -> OpenCV -------------------------------------------------------------------------------------------
def opengl_c2w_to_opencv(c2w):
    """NerfStudioDataLoader.swift:357-366 / BlenderDataLoader.swift:84-88: invert, negate rows 1 and 2 of the
    world-to-camera matrix, invert back (all in f64)."""
    w2c = np.linalg.inv(np.asarray(c2w, np.float64))
    w2c[1:3, :] *= -1
    return np.linalg.inv(w2c)


# ---- NerfStudio (NerfStudioDataLoader.swift) ----------------------------------------------------------------------
def parsePLY(path):
    """:98-215: vertex positions (f32) and colours (u8) of an ascii or binary (x y z r g b, 15-byte vertices) PLY."""
    blob = open(path, "rb").read()
    end = blob.find(b"end_header\n")
    if end < 0:
        raise ValueError("No end_header")
    end += len(b"end_header\n")
    header = blob[:end].decode("ascii")
    line = next((l for l in header.split("\n") if l.startswith("element vertex")), None)
    if line is None:
        raise ValueError("No vertex count")
    n = int(line.split(" ")[-1])
    if "format ascii" in header:
        xyz, rgb = [], []
        for ln in blob[end:].decode("ascii").splitlines()[:n]:
            v = ln.split(" ")
            if len(v) < 6:
                continue
            xyz.append([float(v[0]), float(v[1]), float(v[2])]); rgb.append([int(v[3]), int(v[4]), int(v[5])])
        return np.array(xyz, np.float32).reshape(-1, 3), np.array(rgb, np.uint8).reshape(-1, 3)
    if end + n * 15 > len(blob):
        raise ValueError("File too small")
    rec = np.frombuffer(blob, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]), count=n, offset=end)
    return rec["p"].copy(), rec["c"].copy()


class NerfStudioDataLoader:
    def __init__(self, directory, undistort: bool = False, fisheye=None, normalRoot=None, normalConvention: str = "opencv"):
        """undistort: as ColmapDataLoader's, from the frame's k1, k2, p1, p2 or, when the frame has none of them, the file
        header's; a "camera_model" other than OPENCV or PINHOLE (or none) raises a ValueError in load().
        fisheye: None (the default: exactly the above) or "equidistant", with undistort=True: a frame whose "camera_model" is
        OPENCV_FISHEYE (or SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE) is resampled from its k1 .. k4 (missing ones 0) into the ideal
        equidistant camera and marked "fisheye" in TrainData.cameraModelArray, as ColmapDataLoader's.
        normalRoot, normalConvention: as ColmapDataLoader's; a frame's normal map is <normalRoot>/<the stem of its file_path's
        name>.png."""
        self.directory, self.undistort, self.fisheye = directory, bool(undistort), fisheye
        self.normalRoot, self.normalConvention = normalRoot, normalConvention
        _check_normals(normalRoot, normalConvention, undistort, "NerfStudioDataLoader")
        _check_fisheye(fisheye, undistort, "NerfStudioDataLoader")

    def load(self, resizeFactor: float = 1.0, whiteBackground: bool = False, readImage=readImageRGBA, undistorter=None):
        """loadTrainDataAndPointCloud (:385-416): transforms.json + its ply_file_path.  A frame's "mask_path" (relative to the
        dataset directory, as nerfstudio writes it) is its loss mask (TrainData.maskArray).  undistorter: as
        ColmapDataLoader.load's."""
        meta = json.load(open(os.path.join(self.directory, "transforms.json")))
        xyz, rgb = parsePLY(os.path.join(self.directory, meta["ply_file_path"]))
        ch = rgb.astype(np.float32) / np.float32(255.0)
        pcd = PointCloud(xyz, dict(R=ch[:, 0], G=ch[:, 1], B=ch[:, 2]))

        def intrinsic(d):
            return _intrinsics3(d["fl_x"], d["fl_y"], d["cx"], d["cy"]) if all(k in d for k in ("fl_x", "fl_y", "cx", "cy")) else None
        COEFFS = ("k1", "k2", "p1", "p2")
        intr, c2ws, frames, maskPaths, coeffs, fish = [], [], [], [], [], []
        for fr in meta["frames"]:
            if self.undistort:
                model = fr.get("camera_model", meta.get("camera_model"))
                fish.append(self.fisheye == "equidistant" and model in FISHEYE_MODELS)
                if model not in (None, "OPENCV", "PINHOLE") and not fish[-1]:
                    raise ValueError(f'undistort=True: camera_model "{model}" is not inverted here (OPENCV and PINHOLE are)')
                names = ("k1", "k2", "k3", "k4") if fish[-1] else COEFFS
                src = fr if any(k in fr for k in names) else meta
                coeffs.append([float(src.get(k, 0.0)) for k in names])
            maskPaths.append(os.path.join(self.directory, fr["mask_path"]) if fr.get("mask_path") else None)
            K = intrinsic(fr)
            K = intrinsic(meta) if K is None else K
            if K is None:
                raise ValueError("Failed to load intrinsic matrix")
            if resizeFactor != 1.0:
                K[:2, :3] *= np.float32(resizeFactor)
            intr.append(K)
            frames.append(readImage(os.path.join(self.directory, fr["file_path"]), resizeFactor))
            # the reference reads transform_matrix as Float before widening (:359)
            c2ws.append(opengl_c2w_to_opencv(np.asarray(fr["transform_matrix"], np.float32).astype(np.float64)).astype(np.float32))
        masks = _stack_masks(maskPaths, [f[2] for f in frames], [f[3] for f in frames], resizeFactor)
        models = None
        if self.undistort:
            from .lens import FisheyeLensModel, LensModel
            lenses = [(FisheyeLensModel if f else LensModel)(K[0, 0], K[1, 1], K[0, 2], K[1, 2], *c) for K, c, f in zip(intr, coeffs, fish)]
            frames, masks, _ = _undistort_views(lenses, frames, masks, None, undistorter)
            if any(fish):
                models = np.array(["fisheye" if f else "pinhole" for f in fish])
        Hs, Ws, rgbs, alphas = _stack_frames(frames, whiteBackground)
        td = TrainData(Hs, Ws, np.stack(intr), np.stack(c2ws), rgbs[..., :3], alphas, None, masks)
        td.cameraModelArray = models
        if self.normalRoot is not None:
            stems = [os.path.splitext(os.path.basename(fr["file_path"]))[0] for fr in meta["frames"]]
            td.normalArray = _stack_normals([os.path.join(self.normalRoot, s + ".png") for s in stems], Hs, Ws, resizeFactor,
                                            self.normalConvention)
        return td, pcd, TILE_SIZE_H_W(w=int(Ws[0]) // 4, h=int(Hs[0]) // 4)


# ---- Blender demo set (BlenderDataLoader.swift) --------------------------------------------------------------------
class BlenderDemoDataLoader:
    def __init__(self, folder):
        self.folder = folder

    def readCamera(self):
        """:71-96: info.json -> rgb paths, OpenCV camera-to-world poses, 4x4 intrinsics, max depth."""
        info = json.load(open(os.path.join(self.folder, "info.json")))
        files, poses, intr = [], [], []
        for img in info["images"]:
            files.append(os.path.join(self.folder, img["rgb"]))
            poses.append(opengl_c2w_to_opencv(np.asarray(img["pose"], np.float64)))
            I = np.zeros((4, 4), np.float64)
            I[:3, :3] = np.asarray(img["intrinsic"], np.float64)[:3, :3]
            I[3, 3] = 1
            intr.append(I)
        maxDepth = info["images"][0]["max_depth"] if info["images"] else 1.0
        return files, poses, intr, maxDepth

    def load(self, resizeFactor: float = 1.0, whiteBackground: bool = False):
        """readAll + getPointCloudsFromTrainData (:97-295, :318-341): rgb, <name>_depth.png * max_depth and
        <name>_alpha.png per view; the point cloud is back-projected from the opaque pixels."""
        files, poses, intr, maxDepth = self.readCamera()
        Hs, Ws, rgbs, alphas, depths, Ks = [], [], [], [], [], []
        for path, K in zip(files, intr):
            rgb = _load_image(path, resizeFactor, "RGB")
            base = os.path.splitext(os.path.basename(path))[0].split("_")[0]
            d = os.path.dirname(path)
            depth = _load_image(os.path.join(d, f"{base}_depth.png"), resizeFactor, "L") * np.float32(maxDepth)
            alpha = _load_image(os.path.join(d, f"{base}_alpha.png"), resizeFactor, "L")
            K = K.astype(np.float32)
            if resizeFactor != 1.0:
                K[:2, :3] *= np.float32(resizeFactor)
            if whiteBackground:
                rgb = alpha[..., None] * rgb + (1 - alpha)[..., None]
            Hs.append(rgb.shape[0]); Ws.append(rgb.shape[1]); rgbs.append(rgb); alphas.append(alpha); depths.append(depth); Ks.append(K)
        data = TrainData(np.array(Hs, np.float32), np.array(Ws, np.float32), np.stack(Ks),
                         np.stack([p.astype(np.float32) for p in poses]), np.stack(rgbs).astype(np.float32),
                         np.stack(alphas).astype(np.float32), np.stack(depths).astype(np.float32))
        return data, getPointCloudsFromTrainData(data), TILE_SIZE_H_W(w=int(Ws[0]) // 4, h=int(Hs[0]) // 4)
