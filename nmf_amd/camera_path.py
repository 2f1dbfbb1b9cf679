"""Camera paths for views that are in no data set: a fly-around, a spiral, an interpolation between poses, a path read from a file
(renderer.evaluation_path renders them; `python -m nmf_amd.render --path ...`).  The reference's counterpart is the
`render_path` a data set carries (train.py:884-901 hands it to renderer.evaluation_path); its Blender loader has none.

Everything is built in float64 numpy and returned as [n, 4, 4] float32 camera-to-world matrices in the loader's convention
(BlenderDataset.poses): OpenCV axes -- x right, y down, z forward -- after the Blender flip.  The world is +z up.
"""
import json
import math

import numpy as np

from .dataLoader.blender import BLENDER2OPENCV


def _unit(v, what):
    n = float(np.linalg.norm(v))
    if not n > 1e-12:
        raise ValueError(what)
    return v / n


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """[4, 4] float64 camera-to-world of a camera at `eye` looking at `target`: forward f = normalize(target - eye), right
    r = normalize(f x up), down d = f x r; the rotation's columns are r, d, f and the translation is eye.  A view along `up` has no
    right axis and is refused."""
    eye, target, up = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    f = _unit(target - eye, "look_at: eye and target coincide")
    r = np.cross(f, _unit(up, "look_at: up is zero"))
    if np.linalg.norm(r) < 1e-8:
        raise ValueError("look_at: the view direction is along `up` (the right axis is undefined)")
    r = r / np.linalg.norm(r)
    d = np.cross(f, r)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, d, f, eye
    return c2w


def _on_sphere(center, radius, elevation_deg, azimuth_deg):
    el, az = math.radians(elevation_deg), math.radians(azimuth_deg)
    return np.asarray(center, dtype=np.float64).reshape(3) + radius * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az),
                                                                               math.sin(el)])


def orbit(n, center, radius, elevation_deg, start_deg=0.0):
    """n eyes on the circle of constant elevation around `center`, azimuth start + 360 k / n, looking at `center`: a closed loop
    (frame n would equal frame 0)"""
    if n < 1:
        raise ValueError("orbit: n is at least 1")
    return np.stack([look_at(_on_sphere(center, radius, elevation_deg, start_deg + 360.0 * k / n), center) for k in range(n)]
                    ).astype(np.float32)


def spiral(n, center, radius, elevation_deg, turns=2, radius_scale=(1.0, 1.0)):
    """as orbit with azimuth 360 turns k / n, while elevation (degrees, elevation_deg = (lo, hi)) and radius (radius times
    radius_scale = (lo, hi)) swing as mid + half sin(2 pi k / n) between their ends: closed too"""
    if n < 1:
        raise ValueError("spiral: n is at least 1")
    (e_lo, e_hi), (s_lo, s_hi) = elevation_deg, radius_scale
    out = []
    for k in range(n):
        w = math.sin(2.0 * math.pi * k / n)
        el = 0.5 * (e_lo + e_hi) + 0.5 * (e_hi - e_lo) * w
        rad = radius * (0.5 * (s_lo + s_hi) + 0.5 * (s_hi - s_lo) * w)
        out.append(look_at(_on_sphere(center, rad, el, 360.0 * turns * k / n), center))
    return np.stack(out).astype(np.float32)


def _quat(R):
    """unit quaternion (w, x, y, z) of a rotation matrix, by the largest of the four squared components"""
    t = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1]])
    i = int(np.argmax(t))
    s = 2.0 * math.sqrt(max(1.0 + t[i], 1e-300))
    if i == 0:
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif i == 1:
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif i == 2:
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.asarray(q)
    return q / np.linalg.norm(q)


def _rot(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _slerp(q0, q1, u):
    dot = float(np.dot(q0, q1))
    if dot < 0.0:                                    # the shorter arc
        q1, dot = -q1, -dot
    if dot > 1.0 - 1e-12:
        return q0 + u * (q1 - q0)                    # (normalised by _rot)
    th = math.acos(dot)
    return (math.sin((1.0 - u) * th) * q0 + math.sin(u * th) * q1) / math.sin(th)


def interpolate(keys, n, closed=True):
    """n frames through the K key poses keys [K, 4, 4].  Frame k sits at parameter s = k K / n (closed: the path returns to key 0) or
    k (K - 1) / (n - 1) (open: frame n - 1 is the last key).  The position is the uniform Catmull-Rom spline through the key positions
    (indices wrap when closed, the ends are repeated when open); the rotation is the quaternion SLERP between the two surrounding
    keys on the shorter arc, rebuilt from the unit quaternion: every frame is orthonormal with determinant +1."""
    keys = np.asarray(keys, dtype=np.float64)
    if keys.ndim != 3 or keys.shape[1:] != (4, 4) or keys.shape[0] < 1:
        raise ValueError(f"interpolate: keys is [K, 4, 4], got {keys.shape}")
    if n < 1:
        raise ValueError("interpolate: n is at least 1")
    K = keys.shape[0]
    pos = keys[:, :3, 3]
    quats = [_quat(keys[i, :3, :3]) for i in range(K)]
    at = (lambda i: i % K) if closed else (lambda i: min(max(i, 0), K - 1))
    out = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n):
        s = (k * K) / n if closed else ((k * (K - 1)) / (n - 1) if n > 1 else 0.0)
        i = int(math.floor(s))
        u = s - i
        p0, p1, p2, p3 = (pos[at(i + j)] for j in (-1, 0, 1, 2))
        out[k, :3, 3] = 0.5 * (2.0 * p1 + (p2 - p0) * u + (2.0 * p0 - 5.0 * p1 + 4.0 * p2 - p3) * u * u
                               + (3.0 * p1 - p0 - 3.0 * p2 + p3) * u * u * u)
        out[k, :3, :3] = _rot(_slerp(quats[at(i)], quats[at(i + 1)], u))
    return out.astype(np.float32)


def dataset_orbit(ds):
    """(center [3], radius, elevations in degrees [N]) of a data set's cameras around the centre of its scene_bbox"""
    center = np.asarray(ds.scene_bbox, dtype=np.float64).mean(0)
    rel = np.asarray(ds.poses, dtype=np.float64)[:, :3, 3] - center
    dist = np.linalg.norm(rel, axis=-1)
    return center, float(dist.mean()), np.degrees(np.arcsin(rel[:, 2] / dist))


def from_dataset(ds, kind, n):
    """a path around the scene of a data set: "orbit" at the mean distance and mean elevation of ds.poses from the centre of
    ds.scene_bbox, "spiral" at that distance between the poses' lowest and highest elevation, "interp" through 8 evenly spaced poses
    of the split (all of them if there are fewer), closed"""
    center, radius, elev = dataset_orbit(ds)
    if kind == "orbit":
        return orbit(n, center, radius, float(elev.mean()))
    if kind == "spiral":
        return spiral(n, center, radius, (float(elev.min()), float(elev.max())))
    if kind == "interp":
        poses = np.asarray(ds.poses, dtype=np.float64)
        N = poses.shape[0]
        return interpolate(poses if N <= 8 else poses[(np.arange(8) * N) // 8], n, closed=True)
    raise ValueError(f"from_dataset: kind is orbit, spiral or interp, got '{kind}'")


def save_path(file, c2ws, camera_angle_x, w, h, near_far, intrinsics=None):
    """writes the path as a transforms_*.json in the Blender convention (transform_matrix = c2w @ BLENDER2OPENCV, its own inverse):
    it can be rendered again (load_path), handed to Blender, or written by hand.  intrinsics = (fx, fy, cx, cy) adds fl_x, fl_y, cx,
    cy for cameras camera_angle_x cannot express (load_path prefers them)."""
    c2ws = np.asarray(c2ws)
    if c2ws.ndim != 3 or c2ws.shape[1:] != (4, 4):
        raise ValueError(f"save_path: c2ws is [n, 4, 4], got {c2ws.shape}")
    meta = dict(camera_angle_x=float(camera_angle_x), w=int(w), h=int(h), near_far=[float(near_far[0]), float(near_far[1])])
    if intrinsics is not None:
        meta.update(zip(("fl_x", "fl_y", "cx", "cy"), (float(v) for v in intrinsics)))
    meta["frames"] = [dict(file_path=f"./path/r_{k}", transform_matrix=(c2ws[k].astype(np.float64) @ BLENDER2OPENCV).tolist())
                      for k in range(c2ws.shape[0])]
    with open(file, "w") as f:
        json.dump(meta, f, indent=1)
    return file


def load_path(file, with_camera=False):
    """the poses of a transforms_*.json -> [n, 4, 4] float32, by the loader's arithmetic (on a data set's own file: ds.poses exactly).
    with_camera: -> (poses, dict(w, h, fx, fy, cx, cy, near_far)) with the loader's defaults for what the file leaves out."""
    with open(file) as f:
        meta = json.load(f)
    c2ws = np.stack([(np.array(fr["transform_matrix"], dtype=np.float64) @ BLENDER2OPENCV).astype(np.float32) for fr in meta["frames"]])
    if not with_camera:
        return c2ws
    w, h = int(meta.get("w", 800)), int(meta.get("h", 800))
    if "fl_x" in meta:
        fx, fy = float(meta["fl_x"]), float(meta.get("fl_y", meta["fl_x"]))
    else:
        fx = fy = 0.5 * w / np.tan(0.5 * meta["camera_angle_x"])
    cam = dict(w=w, h=h, fx=fx, fy=fy, cx=float(meta.get("cx", w / 2)), cy=float(meta.get("cy", h / 2)),
               near_far=list(meta.get("near_far", [2.0, 6.0])))
    return c2ws, cam


def dataset_camera(ds):
    """the camera dict of renderer.evaluation_path from a BlenderDataset: its size, focal lengths, centred principal point, near_far"""
    w, h = ds.img_wh
    return dict(w=int(w), h=int(h), fx=float(ds.fx), fy=float(ds.fy), cx=w / 2, cy=h / 2, near_far=list(ds.near_far))
