"""The collision filter's model and world on the host (extension; include/optik_hip.h: the collision filter,
DESIGN.md section 5.12).

A chain of n joint positions has n + 2 frames: 0 the base, k = 1 .. n the pose after joint k's motion, n + 1 the end
effector.  A robot model is a list of spheres, each fixed in one of those frames, a list of self pairs and a margin;
the world is spheres [M, 4] (centre, radius) and oriented boxes [M, 10] (t, unit quaternion i, j, k, w, half
extents) in the base frame.  Everything here only shapes arrays: the distances are computed by the kernels
(csrc/ik_collision.hip), and the arguments are checked again, with the same words, by the C layer.
"""
from __future__ import annotations

import math

import numpy as np

MAX_SPHERES = 256      # OPTIK_HIP_MAX_COLLISION_SPHERES
MAX_PAIRS = 4096       # OPTIK_HIP_MAX_COLLISION_PAIRS
MAX_OBSTACLES = 65536  # OPTIK_HIP_MAX_WORLD_OBSTACLES, of each kind
MAX_GRID_DIM = 1024    # OPTIK_HIP_MAX_GRID_DIM, per axis (at least 2)
MAX_GRID_NODES = 1 << 24  # OPTIK_HIP_MAX_GRID_NODES
MAX_EXCLUDE_SPHERES = 1024  # OPTIK_HIP_MAX_EXCLUDE_SPHERES
MAX_MESH_TRIANGLES = 1 << 20  # OPTIK_HIP_MAX_MESH_TRIANGLES


def auto_pairs(frames):
    """Every sphere pair (a, b), a < b, whose frames differ by 2 or more: spheres on the same or on neighbouring
    frames overlap at the joint between them in every configuration, so they are not checked against each other."""
    f = np.asarray(frames, dtype=np.int64).ravel()
    a, b = np.triu_indices(len(f), k=1)
    keep = np.abs(f[a] - f[b]) >= 2
    return np.stack([a[keep], b[keep]], axis=1).astype(np.int32).reshape(-1, 2)


def model_arrays(frames, centers, radii, self_pairs="auto", margin=0.0):
    """(frames int32 [S], centers [S, 3], radii [S], pairs int32 [P, 2], margin) in the layout of the C ABI.
    self_pairs: "auto" (auto_pairs), None (no pairs) or [P, 2] sphere indices.  Shapes are checked here; values
    (frame range, radii, pair indices, margin) by the C layer."""
    frames = np.ascontiguousarray(np.asarray(frames).ravel(), dtype=np.int32)
    S = len(frames)
    centers = np.ascontiguousarray(np.asarray(centers, dtype=np.float64).reshape(S, 3) if S else np.zeros((0, 3)))
    radii = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float64), (S,)), dtype=np.float64)
    if isinstance(self_pairs, str):
        if self_pairs != "auto":
            raise ValueError("self_pairs must be 'auto', None or a [P, 2] array of sphere indices")
        pairs = auto_pairs(frames)
    elif self_pairs is None:
        pairs = np.zeros((0, 2), dtype=np.int32)
    else:
        pairs = np.asarray(self_pairs)
        if pairs.size and (pairs.ndim != 2 or pairs.shape[1] != 2):
            raise ValueError("self_pairs must be [P, 2] sphere indices")
        pairs = pairs.reshape(-1, 2)
        if pairs.size and not np.issubdtype(pairs.dtype, np.integer):
            raise ValueError("self_pairs must hold integer sphere indices")
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    return frames, centers, radii, pairs, float(margin)


def world_arrays(spheres=None, boxes=None):
    """(spheres [Ms, 4], boxes [Mb, 10]) in the layout of the C ABI; None means none of that kind."""
    sph = np.zeros((0, 4)) if spheres is None else np.asarray(spheres, dtype=np.float64)
    box = np.zeros((0, 10)) if boxes is None else np.asarray(boxes, dtype=np.float64)
    if sph.size == 0:
        sph = np.zeros((0, 4))
    if box.size == 0:
        box = np.zeros((0, 10))
    if sph.ndim != 2 or sph.shape[1] != 4:
        raise ValueError("spheres must be [M, 4]: centre x, y, z, radius")
    if box.ndim != 2 or box.shape[1] != 10:
        raise ValueError("boxes must be [M, 10]: t (3), unit quaternion i, j, k, w (4), half extents (3)")
    return np.ascontiguousarray(sph), np.ascontiguousarray(box)


def grid_arrays(origin, voxel, values=None, shape=None):
    """(origin float64 [3], voxel, values float32 [nx, ny, nz] C-contiguous or None, (nx, ny, nz)) in the layout of the
    C ABI, for the distance-field world: node (i, j, k) sits at origin + voxel * (i, j, k) in
    the base frame.  Give `values` (anything convertible to float32 [nx, ny, nz]) to install a grid, or `shape` alone
    to bake one.  Shapes are checked here; the dimensions' range, the node count, voxel, origin and the values'
    finiteness by the C layer."""
    origin = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).ravel())
    if origin.shape != (3,):
        raise ValueError("origin must be 3 numbers: the position of node (0, 0, 0) in the base frame")
    if values is not None:
        with np.errstate(over="ignore"):  # (a value beyond float32 becomes infinite and is refused by the C layer)
            values = np.ascontiguousarray(np.asarray(values, dtype=np.float32))
        if values.ndim != 3:
            raise ValueError(f"values must be [nx, ny, nz], got {list(values.shape)}")
        if shape is not None and tuple(int(v) for v in shape) != values.shape:
            raise ValueError("shape does not match values")
        shape = values.shape
    elif shape is None:
        raise ValueError("values or shape is needed")
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3:
        raise ValueError("shape must be (nx, ny, nz)")
    return origin, float(voxel), values, shape


def grid_lipschitz(values, voxel):
    """The Lipschitz constant of the trilinear field over `values` [nx, ny, nz] with spacing `voxel`: the square root
    of the sum over the three axes of (the largest absolute difference of neighbouring nodes / voxel)^2 -- inside a
    cell each partial derivative is a convex combination of such differences.  A true distance field gives at most
    sqrt(3), the default of the certified motion check; this is the constant to pass as its
    `grid_lipschitz` for a grid that is not one (a clamped, smoothed or hand-made field)."""
    v = np.asarray(values, dtype=np.float64)
    voxel = float(voxel)
    if v.ndim != 3 or min(v.shape) < 2:
        raise ValueError(f"values must be [nx, ny, nz] with at least 2 nodes per axis, got {list(v.shape)}")
    if not (math.isfinite(voxel) and voxel > 0.0):
        raise ValueError(f"voxel must be finite and > 0, got {voxel!r}")
    total = 0.0
    for axis in range(3):
        g = float(np.abs(np.diff(v, axis=axis)).max()) / voxel
        total += g * g
    return math.sqrt(total)


def default_max_distance(voxel, shape):
    """The grid diagonal voxel * sqrt(nx^2 + ny^2 + nz^2): the clamp of a distance transform that never clamps while
    the grid holds both occupied and free nodes (the largest distance in it is voxel * sqrt(sum (n - 1)^2))."""
    return float(voxel) * math.sqrt(float(sum(int(v) * int(v) for v in shape)))


def occupancy_array(occupied):
    """uint8 [nx, ny, nz], C-contiguous, 1 where `occupied` is non-zero (a bool array, counts, anything numeric)."""
    occupied = np.asarray(occupied)
    if occupied.ndim != 3:
        raise ValueError(f"occupied must be [nx, ny, nz], got {list(occupied.shape)}")
    return np.ascontiguousarray(occupied != 0).view(np.uint8)


def cloud_arrays(points, exclude=None):
    """(points float64 [N, 3], exclude float64 [E, 4]) in the layout of the C ABI; E = 0 without `exclude`."""
    points = np.asarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {list(points.shape)}")
    exclude = np.zeros((0, 4)) if exclude is None else np.asarray(exclude, dtype=np.float64)
    if exclude.size == 0:
        exclude = np.zeros((0, 4))
    if exclude.ndim != 2 or exclude.shape[1] != 4:
        raise ValueError(f"exclude must be [E, 4] (centre, radius), got {list(exclude.shape)}")
    return np.ascontiguousarray(points), np.ascontiguousarray(exclude)


MAP_UNKNOWN = -32768   # OPTIK_HIP_MAP_UNKNOWN: a node of an evidence map that was never observed
MAX_DEPTH_FRAMES = 64  # OPTIK_HIP_MAX_DEPTH_FRAMES
MAX_DEPTH_DIM = 4096   # OPTIK_HIP_MAX_DEPTH_DIM
# The defaults of depth_integrate / set_world_depth: the values with which examples/ik_world_depth.py marks its box
# in one frame and clears it in five, and nothing more -- no sensor was characterised to choose them.
DEPTH_DEFAULTS = dict(z_near=0.1, z_far=4.0, hit=2, miss=1, e_min=-4, e_max=6)
DEPTH_THRESHOLD = 2


def camera_arrays(intrinsics, poses, frames=None):
    """(intrinsics float64 [F, 4], poses float64 [F, 16], each pose a column-major 4x4) in the layout of the C ABI.
    intrinsics: (fx, fy, cx, cy) per frame, [F, 4] or one row for every frame; poses: the camera in the base frame as
    row-major 4x4 matrices (what Robot.fk returns), [F, 4, 4] or one [4, 4].  Shapes are checked here; the values by
    the C layer."""
    poses = np.asarray(poses, dtype=np.float64)
    if poses.shape == (4, 4):
        poses = poses[None]
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        raise ValueError(f"poses must be [F, 4, 4] or one [4, 4], got {list(poses.shape)}")
    F = len(poses) if frames is None else int(frames)
    if len(poses) != F:
        raise ValueError(f"{F} depth images need {F} camera poses, got {len(poses)}")
    intrinsics = np.asarray(intrinsics, dtype=np.float64)
    if intrinsics.shape == (4,):
        intrinsics = np.broadcast_to(intrinsics, (F, 4))
    if intrinsics.shape != (F, 4):
        raise ValueError(f"intrinsics must be [F, 4] (fx, fy, cx, cy) or one such row, got {list(intrinsics.shape)}")
    return np.ascontiguousarray(intrinsics), np.ascontiguousarray(poses.transpose(0, 2, 1)).reshape(F, 16)


def depth_arrays(depth):
    """float32 [F, H, W], C-contiguous, from a stack of depth images or one [H, W] image (F = 1)."""
    depth = np.asarray(depth, dtype=np.float32)
    if depth.ndim == 2:
        depth = depth[None]
    if depth.ndim != 3:
        raise ValueError(f"depth must be [F, H, W] or one [H, W] image, got {list(depth.shape)}")
    return np.ascontiguousarray(depth)


def mesh_arrays(vertices, triangles=None):
    """A mesh as the triangle soup of the C ABI, float64 [M, 9] (the vertices a, b, c of each triangle, base frame),
    C-contiguous.  Either `vertices` [V, 3] with `triangles` [M, 3] integer indices into it (range-checked here), or,
    with `triangles` None, `vertices` [M, 3, 3] (or [M, 9]) as soup already.  Nothing is welded or repaired: the
    winding number needs neither.  Shapes and indices are checked here; the triangle count and the coordinates'
    finiteness by the C layer."""
    v = np.asarray(vertices, dtype=np.float64)
    if triangles is None:
        if not ((v.ndim == 3 and v.shape[1:] == (3, 3)) or (v.ndim == 2 and v.shape[1] == 9)):
            raise ValueError(f"without triangles, vertices must be [M, 3, 3] (a triangle soup), got {list(v.shape)}")
        return np.ascontiguousarray(v.reshape(-1, 9))
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"vertices must be [V, 3], got {list(v.shape)}")
    t = np.asarray(triangles)
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"triangles must be [M, 3] vertex indices, got {list(t.shape)}")
    if not np.issubdtype(t.dtype, np.integer):
        raise ValueError("triangles must hold integer vertex indices")
    if t.size and (int(t.min()) < 0 or int(t.max()) >= len(v)):
        raise ValueError(f"triangles: a vertex index is outside 0..{len(v) - 1}")
    return np.ascontiguousarray(v[t.astype(np.int64)].reshape(-1, 9))


def load_stl(path):
    """The triangles of an STL file as float64 [M, 3, 3] (a soup: nothing is welded, the stored normals are ignored).
    A file is binary (80-byte header, uint32 count, 50-byte records of 12 float32 and 2 attribute bytes) iff its size
    is 84 + 50 * count -- the word "solid" decides nothing, binary files start with it too -- and ASCII otherwise.
    ValueError for a file that is neither (a truncated one, for instance)."""
    with open(path, "rb") as fh:
        data = fh.read()
    if len(data) >= 84:
        count = int(np.frombuffer(data, dtype="<u4", count=1, offset=80)[0])
        if 84 + 50 * count == len(data):
            rec = np.frombuffer(data, dtype=np.dtype([("f", "<f4", (12,)), ("attr", "<u2")]), count=count, offset=84)
            return rec["f"][:, 3:].astype(np.float64).reshape(count, 3, 3)
    try:
        words = data.decode("ascii").split()
    except UnicodeDecodeError:
        raise ValueError(f"{path}: neither a binary STL (84 + 50 * count bytes) nor an ASCII one") from None
    if not words or words[0] != "solid" or "endsolid" not in words:
        raise ValueError(f"{path}: neither a binary STL (84 + 50 * count bytes) nor an ASCII one")
    coords = []
    k, opened, closed = 0, 0, 0
    while k < len(words):
        if words[k] == "vertex":
            try:
                coords.append([float(w) for w in words[k + 1:k + 4]])
            except ValueError:
                raise ValueError(f"{path}: a vertex without three numbers") from None
            if len(coords[-1]) != 3:
                raise ValueError(f"{path}: a vertex without three numbers")
            k += 4
            continue
        opened += words[k] == "facet"
        closed += words[k] == "endfacet"
        k += 1
    if opened != closed or len(coords) != 3 * opened:
        raise ValueError(f"{path}: {opened} facets, {closed} closed, {len(coords)} vertices: not three per facet")
    return np.array(coords, dtype=np.float64).reshape(-1, 3, 3)


def spheres_at(robot, x, frames, centers, radii, pad=0.0, ee_offset=None):
    """The spheres of a model (frames, centers, radii as set_collision_model takes them) in the base frame at the
    configuration x: [S, 4] rows of centre and radius, each radius grown by `pad`.  This is the self-filter's input:
    hand it as `exclude` to occupancy_from_points / set_world_points and the points the camera sees of the robot itself
    are dropped (pad: the sensor's noise plus whatever the sphere model leaves uncovered).  The frames come from
    link_frames_batch_arrays (the GPU); the rotation is done here in numpy."""
    frames = np.asarray(frames, dtype=np.int64).ravel()
    centers = np.asarray(centers, dtype=np.float64).reshape(-1, 3)
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float64), (len(frames),))
    if len(centers) != len(frames):
        raise ValueError("frames, centers and radii must describe the same number of spheres")
    T = robot.link_frames_batch_arrays(np.asarray(x, dtype=np.float64).reshape(1, -1), ee_offset)[0]  # [n + 2, 4, 4]
    if len(frames) and (frames.min() < 0 or frames.max() >= len(T)):
        raise ValueError(f"frames must be in 0..{len(T) - 1}")
    out = np.zeros((len(frames), 4))
    out[:, :3] = np.einsum("sij,sj->si", T[frames, :3, :3], centers) + T[frames, :3, 3]
    out[:, 3] = radii + float(pad)
    return out


def spheres_along_chain(robot, radius, per_link):
    """A sphere model for a chain without collision geometry: spheres of `radius` along every segment between
    consecutive frame origins.  Segment k runs from frame k's origin to frame k + 1's -- the joint origin's offset
    (frame n to n + 1: the tip joint's, without any ee_offset), which does not depend on the configuration -- and
    its spheres sit in frame k.  `per_link` spheres are spread evenly over the part of the segment that keeps 1.5
    radii from both joints; segments shorter than 3 radii get none.  The gap keeps the spheres of two segments joined
    by a zero-length one ("auto" pairs: frames 2 apart) from overlapping in every configuration; the price is that
    the joints themselves and short links (a wrist, a flange) are not covered.  Returns (frames, centers, radii) for
    Robot.set_collision_model."""
    radius = float(radius)
    per_link = int(per_link)
    if not (radius > 0.0) or per_link < 1:
        raise ValueError("radius must be > 0 and per_link >= 1")
    tables = robot.chain_tables()
    origins = np.asarray(tables["origins"])
    gap = 1.5 * radius
    frames, centers = [], []
    for k in range(len(origins)):
        off = origins[k, :3]
        length = float(np.linalg.norm(off))
        if length < 2.0 * gap:
            continue
        fr = [0.5] if per_link == 1 else list(np.linspace(gap / length, 1.0 - gap / length, per_link))
        for s in fr:
            frames.append(k)
            centers.append(s * off)
    frames = np.array(frames, dtype=np.int32)
    centers = np.array(centers, dtype=np.float64).reshape(-1, 3)
    return frames, centers, np.full(len(frames), radius)
