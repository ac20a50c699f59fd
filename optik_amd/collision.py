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


# ---- sphere models from collision geometry ------------------------------------------------

MAX_FIT_SPHERES = 256     # OPTIK_HIP_MAX_FIT_SPHERES: the spheres one fit may choose
MAX_FIT_POINTS = 1 << 20  # OPTIK_HIP_MAX_FIT_POINTS: the surface points one fit may take
# The tessellation of primitive_mesh: a cylinder is a prism over a regular polygon with this many sides, a sphere a
# latitude / longitude polyhedron with this many meridians and half as many bands.  Both are CIRCUMSCRIBED: scaled so
# that the polyhedron contains the true solid; it exceeds it by radius * (1 / cos(pi / 24) - 1) = 0.86 % of the radius
# (cylinder), resp. 1.7 % (sphere).
PRIMITIVE_SEGMENTS = 24
# Robot.fit_spheres' default grid: the longest side of the solid's bounding box is this many voxels.  Nobody has
# measured a good value.  10 makes pad (below) 0.225 of that side, which is coarse; it is chosen so that a handful of
# spheres covers a simple solid completely (uncovered == 0, by the host reference: a 5 : 1 : 1 bar takes 4, a
# cylinder 5, a cube 25 of which the first 8 hold 92 % of the samples).  A finer grid hugs the solid more closely and
# needs many more spheres: at 24 voxels a 2 : 2 : 1 box takes 67.
FIT_VOXELS_PER_EXTENT = 10


def fit_defaults(extent, voxel=None, pad=None, spacing=None):
    """(voxel, pad, spacing) of Robot.fit_spheres for a solid whose bounding box has the longest side `extent`:
    voxel = extent / 10, spacing = voxel / 2, pad = 1.01 * (sqrt(3) * voxel + spacing) -- the 1 % keeps the
    guarantee's condition pad >= sqrt(3) * voxel + spacing (csrc/spherefit_measure.hpp) clear of rounding.  At the
    defaults pad = 0.225 * extent: that is how far a sphere may stick out of the solid.  Values that are given are
    kept; ValueError where they break that condition."""
    extent = float(extent)
    if not (math.isfinite(extent) and extent > 0.0):
        raise ValueError("fit: the solid's bounding box must have a finite, positive extent")
    voxel = extent / FIT_VOXELS_PER_EXTENT if voxel is None else float(voxel)
    if not (math.isfinite(voxel) and voxel > 0.0):
        raise ValueError(f"fit: voxel must be finite and > 0, got {voxel!r}")
    spacing = 0.5 * voxel if spacing is None else float(spacing)
    if not (math.isfinite(spacing) and spacing > 0.0):
        raise ValueError(f"fit: spacing must be finite and > 0, got {spacing!r}")
    need = math.sqrt(3.0) * voxel + spacing
    pad = 1.01 * need if pad is None else float(pad)
    if not (math.isfinite(pad) and pad >= need):
        raise ValueError(f"fit: pad must be >= sqrt(3) * voxel + spacing = {need!r} for every surface point to be "
                         f"coverable, got {pad!r}")
    return voxel, pad, spacing


def fit_grid(lo, hi, voxel, pad):
    """(origin [3], shape) of the grid of Robot.fit_spheres: it contains the bounding box [lo, hi] grown by `pad`."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    origin = lo - pad
    shape = tuple(max(2, int(math.ceil(float(hi[a] + pad - origin[a]) / voxel)) + 1) for a in range(3))
    return origin, shape


def surface_points(vertices, triangles=None, spacing=None):
    """Points on a mesh's surface no further apart than `spacing`, float64 [P, 3]: per triangle (a, b, c) the
    barycentric lattice a + (i / m) (b - a) + (j / m) (c - a), i + j <= m, with m = ceil(longest edge / spacing)
    subdivisions (at least 1).  The lattice cuts the triangle into similar triangles whose edges are at most
    `spacing` long, so every point of the triangle is within `spacing` of a lattice point.  A zero-area triangle
    contributes its vertices (and, where it has length, the lattice along it): nothing divides by an area.  Points
    on shared edges repeat; nothing is merged.  The mesh is given as mesh_arrays takes it.  ValueError above 2^20
    points: raise `spacing`."""
    if spacing is None:
        raise ValueError("surface_points: spacing is needed")
    spacing = float(spacing)
    if not (math.isfinite(spacing) and spacing > 0.0):
        raise ValueError(f"surface_points: spacing must be finite and > 0, got {spacing!r}")
    t = mesh_arrays(vertices, triangles).reshape(-1, 3, 3)
    if not np.isfinite(t).all():
        raise ValueError("surface_points: a NaN or infinite coordinate")
    if len(t) == 0:
        return np.zeros((0, 3))
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    longest = np.sqrt(np.maximum(np.maximum(((b - a) ** 2).sum(1), ((c - b) ** 2).sum(1)), ((a - c) ** 2).sum(1)))
    m = np.maximum(np.ceil(longest / spacing), 1.0)
    total = float(((m + 1.0) * (m + 2.0) / 2.0).sum())
    if total > MAX_FIT_POINTS:
        raise ValueError(f"surface_points: {total:.0f} points at spacing {spacing!r}, more than 2^20: raise spacing")
    m = m.astype(np.int64)
    out = []
    for mm in np.unique(m):
        sel = m == mm
        i, j = np.meshgrid(np.arange(mm + 1), np.arange(mm + 1), indexing="ij")
        keep = (i + j) <= mm
        u, v = i[keep] / float(mm), j[keep] / float(mm)  # [L]
        p = (a[sel][:, None, :] + u[None, :, None] * (b[sel] - a[sel])[:, None, :]
             + v[None, :, None] * (c[sel] - a[sel])[:, None, :])
        out.append((np.nonzero(sel)[0], p))
    # in triangle order
    order = np.argsort(np.concatenate([k for k, _ in out]), kind="stable")
    chunks = [row for _, p in out for row in p]
    return np.ascontiguousarray(np.concatenate([chunks[k] for k in order], axis=0))


def _box_soup(half):
    hx, hy, hz = (float(v) for v in half)
    v = np.array([[(hx if k & 1 else -hx), (hy if k & 2 else -hy), (hz if k & 4 else -hz)] for k in range(8)])
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]  # outward
    return np.array([[v[i], v[j], v[k]] for q in quads for i, j, k in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))])


def primitive_mesh(kind, size):
    """The triangle soup [M, 3, 3] of a URDF collision primitive in its own frame, outward oriented: "box" with size
    (x, y, z) full extents, centred; "cylinder" with size (radius, length), its axis along z, centred; "sphere" with
    size (radius,) or a number.  Cylinder and sphere are tessellated with PRIMITIVE_SEGMENTS = 24 segments and
    circumscribed: the polyhedron contains the true solid (every face plane is at least `radius` from the axis,
    resp. the centre), so a cover of the polyhedron covers the solid."""
    size = np.atleast_1d(np.asarray(size, dtype=np.float64)).ravel()
    if not (np.isfinite(size).all() and (size > 0.0).all()):
        raise ValueError(f"primitive_mesh: {kind} needs finite, positive dimensions, got {size.tolist()}")
    N = PRIMITIVE_SEGMENTS
    if kind == "box":
        if size.shape != (3,):
            raise ValueError("primitive_mesh: a box has size (x, y, z)")
        return _box_soup(0.5 * size)
    if kind == "cylinder":
        if size.shape != (2,):
            raise ValueError("primitive_mesh: a cylinder has size (radius, length)")
        R, h = size[0] / math.cos(math.pi / N), 0.5 * size[1]
        ang = 2.0 * math.pi * np.arange(N) / N
        ring = np.stack([R * np.cos(ang), R * np.sin(ang)], 1)
        tris = []
        for k in range(N):
            (x0, y0), (x1, y1) = ring[k], ring[(k + 1) % N]
            tris += [[[x0, y0, -h], [x1, y1, -h], [x1, y1, h]], [[x0, y0, -h], [x1, y1, h], [x0, y0, h]],
                     [[0.0, 0.0, h], [x0, y0, h], [x1, y1, h]], [[0.0, 0.0, -h], [x1, y1, -h], [x0, y0, -h]]]
        return np.array(tris)
    if kind == "sphere":
        if size.shape != (1,):
            raise ValueError("primitive_mesh: a sphere has size (radius,)")
        nb = N // 2
        lat = math.pi * np.arange(nb + 1) / nb  # polar angle, 0 .. pi
        lon = 2.0 * math.pi * np.arange(N) / N

        def pt(i, k):
            return [math.sin(lat[i]) * math.cos(lon[k % N]), math.sin(lat[i]) * math.sin(lon[k % N]), math.cos(lat[i])]
        tris = []
        for i in range(nb):
            for k in range(N):
                p00, p01, p10, p11 = pt(i, k), pt(i, k + 1), pt(i + 1, k), pt(i + 1, k + 1)
                if i > 0:
                    tris.append([p00, p11, p01])
                if i < nb - 1:
                    tris.append([p00, p10, p11])
        t = np.array(tris)
        # the polyhedron is convex (its quads are planar trapezoids): it contains the ball whose radius is the
        # smallest distance of a face plane from the centre
        n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        d = (n * t[:, 0]).sum(1) / np.linalg.norm(n, axis=1)
        return t * (size[0] / float(d.min()))
    raise ValueError(f"primitive_mesh: kind must be 'box', 'cylinder' or 'sphere', got {kind!r}")


def _rpy_matrix(xyz, rpy):
    r, p, y = (float(v) for v in rpy)
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
    T = np.eye(4)
    T[:3, :3] = [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                 [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                 [-sp, cp * sr, cp * cr]]
    T[:3, 3] = [float(v) for v in xyz]
    return T


def _origin_of(elem):
    o = elem.find("origin") if elem is not None else None
    if o is None:
        return np.eye(4)
    return _rpy_matrix((o.get("xyz") or "0 0 0").split(), (o.get("rpy") or "0 0 0").split())


def default_mesh_resolver(mesh_dir=None):
    """filename -> path: a leading file:// is dropped, a package://name/ prefix is stripped, and what is left is taken
    relative to `mesh_dir` (absolute paths stay)."""
    import os

    def resolve(filename):
        f = filename
        if f.startswith("file://"):
            f = f[len("file://"):]
        if f.startswith("package://"):
            f = f[len("package://"):]
            f = f.split("/", 1)[1] if "/" in f else ""
        return f if os.path.isabs(f) or mesh_dir is None else os.path.join(mesh_dir, f)
    return resolve


def urdf_collision_geometry(urdf_text, base_link, ee_link, mesh_resolver=None, mesh_dir=None, on_missing="raise"):
    """The <collision> geometry of a URDF along the chain base_link -> ee_link, by the chain's frames: (geometry,
    report).  geometry is a list of (frame, kind, T_frame_geom [4, 4], data): kind "box" with data (x, y, z),
    "cylinder" with (radius, length), "sphere" with (radius,), "mesh" with a triangle soup [M, 3, 3] (scale applied,
    in the geometry's own frame); T_frame_geom places the geometry in the frame.

    Frame 0 is the base link and frame k the child link of the k-th moving joint on the path (Robot's frames:
    link_frames_batch_arrays).  A link behind fixed joints belongs to the frame of the last moving joint before it,
    with the fixed transforms accumulated in the URDF's order; where the chain ends in fixed joints, the end link is
    frame n + 1.  Links off the path that hang on a chain link through fixed joints only are included in that link's
    frame; a subtree behind an off-path moving joint (gripper fingers) is skipped and listed in report["skipped"].

    <mesh filename> is resolved by mesh_resolver(filename) -> path (default: default_mesh_resolver(mesh_dir)); only
    .stl is read (load_stl).  Another format or a file that is missing raises ValueError naming the link; with
    on_missing="skip" that geometry is left out and listed in report["skipped"].

    report: "links" (the link of each geometry item), "frames" ({link: frame} of every link that was visited),
    "skipped" (a list of {"link", "reason"}), "joint_origins" ([J, 4, 4]: per moving joint -- and the fixed tip, if
    any -- the transform from the frame before it, fixed joints accumulated in the URDF's order: what the geometry
    is placed by), "fold_order_differs" (the moving joints where the chain loader's fold of fixed joints, which
    multiplies in the other order, gives another origin than the URDF's: there the solver's chain is not the
    URDF's, and the geometry follows the URDF)."""
    import xml.etree.ElementTree as ET
    if on_missing not in ("raise", "skip"):
        raise ValueError("on_missing must be 'raise' or 'skip'")
    resolver = mesh_resolver or default_mesh_resolver(mesh_dir)
    root = ET.fromstring(urdf_text)
    links = {ln.get("name"): ln for ln in root.findall("link")}
    for name in (base_link, ee_link):
        if name not in links:
            raise ValueError(f"link '{name}' does not exist")
    joints = []
    for j in root.findall("joint"):
        joints.append(dict(name=j.get("name"), type=j.get("type"), parent=j.find("parent").get("link"),
                           child=j.find("child").get("link"), T=_origin_of(j)))
    children = {}
    for k, j in enumerate(joints):
        children.setdefault(j["parent"], []).append(k)
    # breadth-first path, as the chain loader finds it
    via = {base_link: None}
    queue = [base_link]
    while queue and ee_link not in via:
        u = queue.pop(0)
        for k in children.get(u, []):
            if joints[k]["child"] not in via:
                via[joints[k]["child"]] = k
                queue.append(joints[k]["child"])
    if ee_link not in via:
        raise ValueError("no path from base to EE link")
    path = []
    u = ee_link
    while via[u] is not None:
        path.insert(0, via[u])
        u = joints[via[u]]["parent"]
    on_path = set(path)
    n = sum(joints[k]["type"] != "fixed" for k in path)

    placed = [(base_link, 0, np.eye(4))]  # (link, frame, T_frame_link) along the path
    frame, T = 0, np.eye(4)
    acc_true, acc_loader = np.eye(4), np.eye(4)
    joint_origins, differs = [], []
    for k in path:
        j = joints[k]
        if j["type"] == "fixed":
            T = T @ j["T"]
            acc_true, acc_loader = acc_true @ j["T"], j["T"] @ acc_loader
        else:
            frame += 1
            origin_true, origin_loader = acc_true @ j["T"], j["T"] @ acc_loader
            joint_origins.append(origin_true)
            if not np.allclose(origin_true, origin_loader, rtol=0.0, atol=1e-12):
                differs.append(j["name"])
            T, acc_true, acc_loader = np.eye(4), np.eye(4), np.eye(4)
        placed.append((j["child"], frame, T.copy()))
    if path and joints[path[-1]]["type"] == "fixed" and not np.array_equal(acc_loader, np.eye(4)):
        # the chain's fixed tip: the end link is frame n + 1
        joint_origins.append(acc_true)
        if not np.allclose(acc_true, acc_loader, rtol=0.0, atol=1e-12):
            differs.append(joints[path[-1]]["name"])
        placed[-1] = (ee_link, n + 1, np.eye(4))

    report = dict(links=[], frames={}, skipped=[], joint_origins=np.array(joint_origins).reshape(-1, 4, 4),
                  fold_order_differs=differs)
    visit = []
    for link, f, Tl in placed:
        visit.append((link, f, Tl))
        stack = [(link, f, Tl)]
        while stack:  # off-path subtrees
            u, fu, Tu = stack.pop()
            for k in children.get(u, []):
                if k in on_path:
                    continue
                j = joints[k]
                if j["type"] == "fixed":
                    item = (j["child"], fu, Tu @ j["T"])
                    visit.append(item)
                    stack.append(item)
                else:
                    report["skipped"].append(dict(link=j["child"], reason=f"behind the off-chain {j['type']} joint "
                                                                          f"'{j['name']}': moving links off the chain are not modelled"))
    geometry = []
    for link, f, Tl in visit:
        report["frames"][link] = f
        for col in links[link].findall("collision") if link in links else []:
            g = col.find("geometry")
            shape = list(g)[0] if g is not None and len(g) else None
            if shape is None:
                continue
            Tg = Tl @ _origin_of(col)
            if shape.tag == "box":
                item = ("box", np.array([float(v) for v in shape.get("size").split()]))
            elif shape.tag == "cylinder":
                item = ("cylinder", np.array([float(shape.get("radius")), float(shape.get("length"))]))
            elif shape.tag == "sphere":
                item = ("sphere", np.array([float(shape.get("radius"))]))
            elif shape.tag == "mesh":
                import os
                filename = shape.get("filename") or ""
                path_ = resolver(filename)
                why = None
                if not filename.lower().endswith(".stl"):
                    why = f"link '{link}': collision mesh '{filename}' is not an .stl file (the only format read)"
                elif not (path_ and os.path.isfile(path_)):
                    why = f"link '{link}': collision mesh '{filename}' not found (looked for {path_!r})"
                if why:
                    if on_missing == "raise":
                        raise ValueError(why)
                    report["skipped"].append(dict(link=link, reason=why))
                    continue
                soup = load_stl(path_)
                scale = np.array([float(v) for v in (shape.get("scale") or "1 1 1").split()])
                item = ("mesh", soup * scale)
            else:
                report["skipped"].append(dict(link=link, reason=f"link '{link}': unknown geometry <{shape.tag}>"))
                continue
            geometry.append((f, item[0], Tg, item[1]))
            report["links"].append(link)
    return geometry, report


def geometry_soup(kind, T, data):
    """One item of urdf_collision_geometry as a triangle soup [M, 3, 3] in its frame (primitive_mesh, resp. the mesh
    itself, moved by T)."""
    soup = np.asarray(data, dtype=np.float64).reshape(-1, 3, 3) if kind == "mesh" else primitive_mesh(kind, data)
    T = np.asarray(T, dtype=np.float64)
    return soup @ T[:3, :3].T + T[:3, 3]


def mid_configuration(robot):
    """The middle of the joint range, [n] (a joint without finite limits: 0)."""
    lb, ub = (np.asarray(v, dtype=np.float64) for v in robot.joint_limits())
    mid = 0.5 * (lb + ub)
    return np.where(np.isfinite(mid), mid, 0.0)


def prune_pairs(robot, frames, centers, radii, pairs, configs=None, margin=0.0):
    """(kept [Pk, 2], dropped [Pd, 2]) int32: `pairs` without the sphere pairs that overlap -- their distance less
    the two radii is below `margin` -- at any of the reference configurations `configs` [B, n] (default: the middle
    of the joint range).  Padded spheres on frames two apart can overlap in every configuration; a model that keeps
    such a pair is always in self-collision.  A pair that overlaps at a configuration the robot may take is taken to
    be of that kind: the reference configurations have to be free of real self-collision.  The frames come from
    link_frames_batch_arrays (the GPU); the rest is numpy."""
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    configs = mid_configuration(robot)[None] if configs is None else np.asarray(configs, dtype=np.float64)
    configs = configs.reshape(-1, robot.num_positions())
    overlap = np.zeros(len(pairs), dtype=bool)
    for x in configs:
        s = spheres_at(robot, x, frames, centers, radii)
        d = np.linalg.norm(s[pairs[:, 0], :3] - s[pairs[:, 1], :3], axis=1) - s[pairs[:, 0], 3] - s[pairs[:, 1], 3]
        overlap |= d < float(margin)
    return np.ascontiguousarray(pairs[~overlap]), np.ascontiguousarray(pairs[overlap])
