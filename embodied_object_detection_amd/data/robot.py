"""Robot online front-end: second caller of the model boundary.

Mirrors the per-frame preparation of `Detic/robot_demo.py:489-534` and `EmbodiedPredictor.__call__`
(`Detic/detic/predictor.py:406-439`): nearest-timestamp association of RGB / depth / pose files, depth in millimetres -> metres,
the fixed RealSense intrinsics, the axis-swapped camera transform `T @ R` (`robot_demo.py:40-90`), grid-cell indexing with the
robot's `x * map_h + y` ordering (`robot_demo.py:533`), and the frame dict the model takes.  `RobotFrontEnd` takes arrays; `RobotRun` reads a recorded run from disk (16-bit depth PNGs and
RGB images through Pillow, poses through numpy).  The un-projection + indexing runs in the HIP kernel (`order=1`).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

# `ProjectorUtils.compute_intrinsic_matrix` of robot_demo.py:124-126 (fixed K, not derived from the fov)
ROBOT_INTRINSICS = (np.float32(380.3127746582031), np.float32(379.828857421875), np.float32(315.81829833984375),
                    np.float32(250.9555206298828))
ROBOT_MAP_SHIFT = (-13.0, 0.0, -13.0)     # robot_demo.py:476
ROBOT_RES = 0.2                            # robot_demo.py:470
ROBOT_MAP_W = ROBOT_MAP_H = math.ceil(40 / ROBOT_RES)   # 200 x 200 (robot_demo.py:471-474)
ROBOT_CAMERA_HEIGHT = 0.65
ROBOT_ELEVATION = math.pi + 0.06


def nearest_by_timestamp(stamp: int, candidates: Sequence[str]) -> str:
    """`min(files, key=|int(stem) - t|)` (robot_demo.py:493-496); first minimum wins, like Python's `min`."""
    return min(candidates, key=lambda x: abs(int(x.split(".")[0]) - int(stamp)))


def robot_transform(pose_xyt: Sequence[float]) -> np.ndarray:
    """`_transform3D(xyzhe) @ R` of robot_demo.py:40-90 with xyzhe = (x, 0.65, y, -theta, pi + 0.06) (robot_demo.py:519), fp32."""
    x, y, th = [np.float32(v) for v in pose_xyt[:3]]
    heading, elev = np.float32(-th), np.float32(ROBOT_ELEVATION)
    cx, sx = np.cos(elev, dtype=np.float32), np.sin(elev, dtype=np.float32)
    cy, sy = np.cos(heading, dtype=np.float32), np.sin(heading, dtype=np.float32)
    T = np.zeros((4, 4), dtype=np.float32)
    T[0] = [cy, sx * sy, cx * sy, x]
    T[1] = [0, cx, -sx, np.float32(ROBOT_CAMERA_HEIGHT)]
    T[2] = [-sy, cy * sx, cy * cx, y]
    T[3, 3] = 1
    R = np.zeros((4, 4), dtype=np.float32)
    R[0, 2] = R[1, 1] = R[2, 0] = R[3, 3] = 1
    return (T @ R).astype(np.float32)


class RobotFrontEnd:
    """Builds model inputs from raw robot frames; one instance per run (the memory grid is fixed at 200 x 200 @ 0.2 m)."""

    def __init__(self, projector: Optional[Callable] = None, map_w: int = ROBOT_MAP_W, map_h: int = ROBOT_MAP_H,
                 res: float = ROBOT_RES, map_shift=ROBOT_MAP_SHIFT, sequence_name: str = "robot"):
        self.projector = projector
        self.map_w, self.map_h, self.res = map_w, map_h, float(res)
        self.map_shift = np.asarray(map_shift, dtype=np.float32)
        self.n_cells = map_w * map_h
        self.sequence_name = sequence_name
        self._first = True

    def frame(self, rgb_hwc_u8: np.ndarray, depth_mm: np.ndarray, pose_xyt: Sequence[float], file_name: str = "",
              heights: bool = False) -> Dict:
        """The frame dict the model takes.  `heights=True` adds `"heights"`, float32 [H, W]: the world y of every pixel in metres,
        from the same launch that makes `proj_indices` (for `heights` of the model and the predictor); a `projector` of the
        caller's own must then take `want_xyz=True` and say so with an attribute `returns_xyz = True` (`synthetic.hip_projector`
        does), otherwise the call raises.  The default leaves the dict as it always was."""
        if self.projector is None:
            from .synthetic import hip_projector
            self.projector = hip_projector()
        if heights and not getattr(self.projector, "returns_xyz", False):
            raise ValueError("RobotFrontEnd.frame(heights=True): the projector cannot return heights (it needs a want_xyz argument "
                             "and the attribute returns_xyz = True, as synthetic.hip_projector has)")
        H, W = depth_mm.shape
        # robot_demo.py:515-517: uint16 millimetres / 1000 in float64, then FloatTensor (one rounding to fp32)
        depth_m = (np.asarray(depth_mm, dtype=np.float64) / 1000).astype(np.float32)
        T = robot_transform(pose_xyt)
        args = (depth_m, T, ROBOT_INTRINSICS, (0.0, 0.0, 0.0), self.map_shift, self.res, self.map_w, self.map_h, 1)
        if heights:
            proj, xyz = self.projector(*args, want_xyz=True)
        else:
            proj = self.projector(*args)
        image = torch.from_numpy(np.ascontiguousarray(np.asarray(rgb_hwc_u8).transpose(2, 0, 1)))
        reset, self._first = self._first, False
        out = {"image": image, "height": H, "width": W, "proj_indices": np.ascontiguousarray(proj, dtype=np.int32).reshape(H, W, 1),
               "memory": np.zeros((self.n_cells, 1), dtype=np.float32), "memory_reset": reset,
               "sequence_name": self.sequence_name, "observations": None, "file_name": file_name}
        if heights:
            out["heights"] = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(H, W, 3)[:, :, 1])
        return out

    def robot_cell(self, pose_xyt: Sequence[float]) -> Tuple[int, int]:
        """Robot position on the map (robot_demo.py:536-538)."""
        p = (np.asarray(pose_xyt[:2], dtype=np.float32) - self.map_shift[[0, 2]]) / np.float32(self.res)
        q = np.rint(p).astype(np.int64)
        return int(q[0]), int(q[1])

    def cell_center(self, cell) -> Tuple[float, float]:
        """The inverse of `robot_cell`: the (x, y) in metres of the middle of a cell, given as the pair `robot_cell` returns or as the
        memory's index `x * map_h + y` (a peak of `locate` with `map_shape=(map_w, map_h)`)."""
        cx, cy = divmod(int(cell), self.map_h) if np.ndim(cell) == 0 else (int(cell[0]), int(cell[1]))
        return (float(cx * self.res + float(self.map_shift[0])), float(cy * self.res + float(self.map_shift[2])))


    def cell_centers(self, cells) -> np.ndarray:
        """`cell_center` for many memory indices `x * map_h + y` at once (the `cells` of `place`, the `peaks` of `locate`, the
        `reach_cell` of `frontiers`: the known free cell to drive to for a look beyond a frontier): float64 [n, 2] in metres, NaN for
        the padding value -1."""
        c = np.asarray(cells.cpu() if torch.is_tensor(cells) else cells, dtype=np.int64).reshape(-1)
        cx, cy = np.divmod(c, self.map_h)
        out = np.stack([cx * self.res + float(self.map_shift[0]), cy * self.res + float(self.map_shift[2])], axis=1).astype(np.float64)
        out[c < 0] = np.nan
        return out

    def region_centroids(self, sum_rc, area) -> np.ndarray:
        """The centroids of the regions of `regions(..., map_shape=(map_w, map_h))` in metres: `sum_rc` [..., 2] over `area` [...],
        with the index convention of `cell_center` (cell = x * map_h + y, so the row is x and the column is y).  float64 [..., 2];
        NaN for the padding (area 0).  The `sum_rc` and `area` of `inventory(..., map_shape=(map_w, map_h))` are served alike: its
        objects are summed the same way, [K, 2] over [K] (or [B, K, 2] over [B, K])."""
        s = np.asarray(sum_rc.cpu() if torch.is_tensor(sum_rc) else sum_rc, dtype=np.float64)
        a = np.asarray(area.cpu() if torch.is_tensor(area) else area, dtype=np.float64)
        if s.shape != a.shape + (2,):
            raise ValueError(f"region_centroids: sum_rc {s.shape} against area {a.shape}")
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = np.where(a[..., None] > 0, s / a[..., None], np.nan)
        return np.stack([mean[..., 0] * self.res + float(self.map_shift[0]), mean[..., 1] * self.res + float(self.map_shift[2])], axis=-1)

    def relation_metres(self, d2) -> np.ndarray:
        """The squared cell distances of `relations` (`min_d2`, `nearest_d2`, `from_d2`) in metres: sqrt(d2) * res as float64 in the
        shape of `d2`; inf for INT_MAX (no pair within reach, an empty slot, no `from_cell`).  The point to drive to is
        `cell_centers(rel["from_closest"])`.  The `reach_cost` of `frontiers` goes through here when it is a squared distance
        (`from_cell` given, no `route`)."""
        d = np.asarray(d2.cpu() if torch.is_tensor(d2) else d2, dtype=np.int64)
        return np.where(d == 2 ** 31 - 1, np.inf, np.sqrt(d.astype(np.float64)) * self.res)

    def route_metres(self, cost) -> np.ndarray:
        """The costs of `route` (`dist`, `goal_cost`) in metres: cost / 5 * res as float64 in the shape of `cost` (a move along a
        row or column costs 5, a diagonal one 7); inf for INT_MAX (blocked, unreached, no way to the object).  The waypoints are
        `cell_centers(route["path"][k])`, NaN behind the path's end.  The `reach_cost` of `frontiers(..., route=rt)` is such a
        cost, taken from `rt["dist"]`; the centroid of a frontier is `region_centroids(fr["sum_rc"], fr["area"])`."""
        d = np.asarray(cost.cpu() if torch.is_tensor(cost) else cost, dtype=np.int64)
        return np.where(d == 2 ** 31 - 1, np.inf, d.astype(np.float64) / 5.0 * self.res)

    def clearance_metres(self, d2) -> np.ndarray:
        """The squared cell distances of `clearance` (`d2`, `widest_d2`) in metres: sqrt(d2) * res as float64 in the shape of `d2`;
        inf for INT_MAX (the map has no blocked cell).  The most open place is `cell_centers(clr["widest_cell"])`; whether the
        object is in view from it is `sight`'s to say."""
        d = np.asarray(d2.cpu() if torch.is_tensor(d2) else d2, dtype=np.int64)
        return np.where(d == 2 ** 31 - 1, np.inf, np.sqrt(d.astype(np.float64)) * self.res)

    def body_radius2(self, metres: float) -> int:
        """The `radius2` of `clearance` and the `body_radius2` of `route` for a body of radius `metres`: the radius in cells,
        squared and rounded down (1e-9 keeps a radius that is a whole number of cells from falling short by rounding)."""
        return int(np.floor((float(metres) / self.res) ** 2 + 1e-9))

    def door_r2(self, width_m: float) -> int:
        """The `door_r2` of `rooms` for doorways up to `width_m` metres wide: half the width in cells, squared and rounded down, as
        `body_radius2` rounds.  A free cell at most that far (squared) from a wall is no core of a room, so an opening up to
        about that wide divides two rooms and a wider one joins them."""
        return int(np.floor((float(width_m) / (2.0 * self.res)) ** 2 + 1e-9))

    def sight_range2(self, metres: float) -> int:
        """The `range2` of `sight` for a sensor that reaches `metres`: the range in cells, squared and rounded down, as
        `body_radius2` rounds, and INT_MAX (unbounded) from there on.  The `near_d2` of `sight` in metres is
        `relation_metres(near_d2)`."""
        return int(min(np.floor((float(metres) / self.res) ** 2 + 1e-9), 2 ** 31 - 1))

    def height_band_mm(self, lo_m: float, hi_m: float) -> Tuple[int, int]:
        """The `band_mm` of `heights` for a body that clears what is lower than `lo_m` and passes under what is higher than `hi_m`
        (metres above the world's zero, the floor the camera height `ROBOT_CAMERA_HEIGHT` is measured from): whole millimetres,
        rounded to nearest."""
        lo, hi = int(round(float(lo_m) * 1000.0)), int(round(float(hi_m) * 1000.0))
        if not -1000000 <= lo <= hi <= 1000000:
            raise ValueError(f"height_band_mm: {lo_m} .. {hi_m} m: expected lo <= hi within +-1000 m")
        return lo, hi

    def exclude_cell(self, pose_xyt: Sequence[float]) -> int:
        """The robot's own cell as the memory's index `x * map_h + y`: the `exclude_cell` of `place`."""
        x, y = self.robot_cell(pose_xyt)
        return x * self.map_h + y


def read_depth_mm(path: str) -> np.ndarray:
    """`cv2.imread(path, cv2.IMREAD_ANYDEPTH)` (robot_demo.py:498): the 16-bit depth PNG as uint16 millimetres, via Pillow."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.ndim != 2:
        raise ValueError(f"{path}: expected a single-channel depth image, got shape {a.shape}")
    return a.astype(np.uint16) if a.dtype != np.uint16 else a


def read_rgb(path: str) -> np.ndarray:
    """The Detic loader's own decode, inlined at robot_demo.py:503-507: Pillow, EXIF orientation, RGB uint8 HWC."""
    from PIL import Image, ImageOps
    with Image.open(path) as im:
        return np.asarray(ImageOps.exif_transpose(im).convert("RGB"))


class RobotRun:
    """One recorded robot run on disk (`<root>/images`, `<root>/depth`, `<root>/pose`, file stems = timestamps): every second RGB
    image (~10 Hz) with the depth image and the odometry sample closest in time (robot_demo.py:485-499), turned into model frames
    by a `RobotFrontEnd`."""

    def __init__(self, root: str, front_end: Optional[RobotFrontEnd] = None, every: int = 2):
        import os
        self.root = root
        self.images = sorted(os.listdir(os.path.join(root, "images")))
        self.depth = sorted(os.listdir(os.path.join(root, "depth")))
        self.pose = sorted(os.listdir(os.path.join(root, "pose")))
        self.every = every
        self.front_end = front_end or RobotFrontEnd(sequence_name=os.path.basename(os.path.normpath(root)))

    def __len__(self) -> int:
        return len(self.images[::self.every])

    def __iter__(self):
        import os
        for image in self.images[::self.every]:
            stamp = image.split(".")[0]
            d = nearest_by_timestamp(stamp, self.depth)
            p = nearest_by_timestamp(stamp, self.pose)
            depth_mm = read_depth_mm(os.path.join(self.root, "depth", d))
            pose = np.load(os.path.join(self.root, "pose", p))
            rgb = read_rgb(os.path.join(self.root, "images", image))
            f = self.front_end.frame(rgb, depth_mm, pose, file_name=image)
            f["depth_file"], f["pose_file"] = d, p
            yield f
