"""Host-side camera, mirroring the reference's `Camera`
(Trainer/CameraUtil.swift:5-102, Trainer/simd+ext.swift:45-66).

view  = (c2w^-1)^T stored row-major, so p_view = [p, 1] @ view (translation in row 3)
proj  = rows (2n/(r-l),0,0,0), (0,2n/(t-b),0,0), (0,0,f/(f-n),1), (0,0,-nf/(f-n),0)
FoV   = 2 atan(pixels / (2 focal)) evaluated in f32; matrices built in f64, cast to f32.
The reference ignores the principal point (CameraUtil.swift:26-27); here it is optional: Camera(cx=, cy=)
puts offX = (2 cx - W) / W, offY = (2 cy - H) / H into row 2 of proj, so that a view-space point (x, y, z) lands at
means2d = (fx x / z + cx - 0.5, fy y / z + cy - 0.5): pixel i covers [i, i + 1), COLMAP's and nerfstudio's convention.  Without
cx, cy the camera is the reference's centred one, bit for bit.
"""
from __future__ import annotations

import numpy as np


def simd_to_row_major(columns) -> np.ndarray:
    """simd_float4x4 / simd_double4x4 `toMLXArray()` (Trainer/simd+ext.swift:45-55): simd stores COLUMNS
    (`m[c][r]`, `m[c, r]` is element (r, c)); the array handed to the kernels is row-major with a[r][c] = m[c][r].
    With that layout a simd `v * m` (row vector times matrix) is `v @ a`, which is why the kernels compute
    p_view = [p, 1] @ view with the translation in row 3."""
    cols = np.asarray(columns)
    return np.ascontiguousarray(cols.T)


def focal2fov(focal: float, pixels: float) -> np.float32:
    return np.float32(2.0) * np.arctan(np.float32(pixels) / (np.float32(2.0) * np.float32(focal)))


def fov2focal(fov: float, pixels: float) -> float:
    return pixels / (2.0 * np.tan(fov / 2.0))


def getProjectionMatrix(znear: float, zfar: float, fovX: float, fovY: float, offX: float = 0.0, offY: float = 0.0) -> np.ndarray:
    """Row-major array the reference hands to its kernels (P.transpose.toMLXArray()).  offX = (2 cx - W) / W and offY =
    (2 cy - H) / H move the principal point off the centre: with this code base's clip w = +z the off-centre term
    -(r + l) / (r - l) of the frustum is +offX (Inria's w = -z form carries the other sign and would mirror the shift)."""
    tanHalfY, tanHalfX = np.tan(fovY / 2.0), np.tan(fovX / 2.0)
    top, right = tanHalfY * znear, tanHalfX * znear
    bottom, left = -top, -right
    P = np.zeros((4, 4), np.float64)
    P[0, 0] = 2 * znear / (right - left)
    P[1, 1] = 2 * znear / (top - bottom)
    P[2, 0] = (right + left) / (right - left) + offX       # (the symmetric frustum's 0, plus the offset)
    P[2, 1] = (top + bottom) / (top - bottom) + offY
    P[2, 2] = zfar / (zfar - znear)
    P[2, 3] = 1.0
    P[3, 2] = -znear * zfar / (zfar - znear)
    return P


CAMERA_MODELS = {"pinhole": 0, "fisheye": 1}      # GS_CAMERA_PINHOLE, GS_CAMERA_FISHEYE (include/gsplat.h)


class Camera:
    def __init__(self, width: int, height: int, focalX: float, focalY: float, c2w, znear: float = 0.1,
                 zfar: float = 100.0, cx: float | None = None, cy: float | None = None, model: str = "pinhole"):
        """model: "pinhole" (the default: every field is what it is without the argument) or "fisheye", the ideal equidistant
        camera (include/gsplat.h gs_set_camera_model): focalX, focalY, cx, cy and the pose mean what they
        mean for a pinhole, a point at angle theta off the axis lands focal * theta from the principal point, and FoVx / FoVy
        and the rest of the projection matrix are not read by the renderer.
        cx, cy: the principal point in pixels (pixel i covers [i, i + 1)); None is the image centre W / 2, H / 2, and then
        every field is the reference's.  FoVx / FoVy stay 2 atan(pixels / (2 focal)): they feed the EWA clamp's symmetric
        limX / limY, which the principal point does not enter."""
        if model not in CAMERA_MODELS:
            raise ValueError(f"Camera: model is one of {sorted(CAMERA_MODELS)}")
        self.model = model
        c2w = np.asarray(c2w, dtype=np.float64).reshape(4, 4)
        self.imageWidth, self.imageHeight = int(width), int(height)
        self.focalX, self.focalY = np.float32(focalX), np.float32(focalY)
        self.FoVx = focal2fov(self.focalX, float(width))
        self.FoVy = focal2fov(self.focalY, float(height))
        # simd_double4x4.fromMlxArray(c2w).inverse.transpose.toMLXArray() (CameraUtil.swift:30, :34): fromMlxArray /
        # toMLXArray are the row-major <-> column-storage pair above, so in array terms this is inv(c2w)^T
        self.worldViewTransform = np.ascontiguousarray(np.linalg.inv(c2w).T.astype(np.float32))
        self.principalX = float(width) / 2.0 if cx is None else float(cx)
        self.principalY = float(height) / 2.0 if cy is None else float(cy)
        offX = (2.0 * self.principalX - float(width)) / float(width)
        offY = (2.0 * self.principalY - float(height)) / float(height)
        self.projectionMatrix = np.ascontiguousarray(
            getProjectionMatrix(znear, zfar, float(self.FoVx), float(self.FoVy), offX, offY).astype(np.float32))
        self.cameraCenter = c2w[:3, 3].copy()
        self.c2w = c2w.copy()

    def as_dict(self):
        d = dict(view=self.worldViewTransform, proj=self.projectionMatrix, fovX=float(self.FoVx),
                 fovY=float(self.FoVy), focalX=float(self.focalX), focalY=float(self.focalY),
                 camCenter=self.cameraCenter.astype(np.float32), principalX=self.principalX, principalY=self.principalY)
        if self.model != "pinhole":
            d["model"] = self.model
        return d


def look_at_c2w(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)) -> np.ndarray:
    """OpenCV-convention camera-to-world (x right, y down, z forward)."""
    eye = np.asarray(eye, np.float64)
    fwd = np.asarray(target, np.float64) - eye
    fwd /= np.linalg.norm(fwd)
    upv = np.asarray(up, np.float64)
    right = np.cross(fwd, upv)
    if np.linalg.norm(right) < 1e-8:
        right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, down, fwd, eye
    return c2w


def _skew(w) -> np.ndarray:
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def rodrigues(w) -> np.ndarray:
    """R(w) = I + A [w]x + B [w]x^2, A = sin t / t, B = (1 - cos t) / t^2, t = |w|; their series below t^2 = 1e-3, so that
    R(0) is exactly I (include/gsplat.h gs_set_pose_correction)."""
    w = np.asarray(w, np.float64).reshape(3)
    t2 = float(w @ w)
    if t2 < 1e-3:
        A, B = 1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0
    else:
        t = np.sqrt(t2)
        A, B = np.sin(t) / t, 2.0 * np.sin(0.5 * t) ** 2 / t2
    K = _skew(w)
    return np.eye(3) + A * K + B * (K @ K)


def pose_delta_matrix(delta) -> np.ndarray:
    """dT(delta) = [[R(w), tau], [0, 1]] for delta = (w, tau) in R^6."""
    d = np.asarray(delta, np.float64).reshape(6)
    T = np.eye(4)
    T[:3, :3] = rodrigues(d[:3])
    T[:3, 3] = d[3:]
    return T


def apply_pose_correction(camera: Camera, delta) -> Camera:
    """The camera with its pose corrected by delta = (w, tau), in float64: c2w' = c2w dT(delta), the correction acting in the
    camera's own OpenCV frame (x right, y down, z forward).  Intrinsics and the projection matrix are the camera's own.  What
    the renderer composes on the device while a correction is set (GaussianRenderer.setPoseCorrection), and how a trainer's
    refined cameras are exported (GaussianTrainer.refinedCamera)."""
    c2w = getattr(camera, "c2w", None)
    if c2w is None:
        c2w = np.linalg.inv(np.asarray(camera.worldViewTransform, np.float64).T)
    out = Camera(camera.imageWidth, camera.imageHeight, camera.focalX, camera.focalY, np.asarray(c2w, np.float64) @ pose_delta_matrix(delta),
                 cx=getattr(camera, "principalX", None), cy=getattr(camera, "principalY", None), model=getattr(camera, "model", "pinhole"))
    out.projectionMatrix = camera.projectionMatrix.copy()
    return out


def cameras_from_train_data(trainData, principal_point: bool = True, znear: float = 0.1, zfar: float = 100.0):
    """[Camera] of a loader's TrainData (Hs, Ws, intrinsicArray, c2wArray): focal lengths and, with principal_point, cx, cy from
    each view's intrinsics -- the camera model pointcloud.getRaysFromImages back-projects with.  principal_point=False gives
    the reference's centred cameras.  A view marked "fisheye" in trainData.cameraModelArray (the loaders' fisheye="equidistant")
    becomes a Camera(model="fisheye")."""
    Hs, Ws, intr, c2ws = trainData.getCameraParams()
    models = getattr(trainData, "cameraModelArray", None)
    cams = []
    for i, (H, W, K, c2w) in enumerate(zip(Hs, Ws, np.asarray(intr, np.float64), np.asarray(c2ws, np.float64))):
        cx, cy = (float(K[0, 2]), float(K[1, 2])) if principal_point else (None, None)
        cams.append(Camera(int(W), int(H), K[0, 0], K[1, 1], c2w, znear, zfar, cx=cx, cy=cy,
                           model="pinhole" if models is None else str(models[i])))
    return cams
