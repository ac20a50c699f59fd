#!/usr/bin/env python3
"""Cost of depth-image worlds; writes profiles/depth_cost.txt.

The scene is section 5.12's (tools/grid_cost.py: world_a, 64 spheres and 16 boxes), rendered in numpy to a 480 x 640
z-depth image from one camera pose, over grids of 128^3 (voxel 0.02) and 256^3 (voxel 0.01) on the same volume.  Per
grid, interleaved in one process, medians of --reps (7) after a warm-up round, with [min, max]:

  integrate1   HipChain.depth_integrate of one frame (device buffers)
  integrate8   HipChain.depth_integrate of eight frames in one call (the same image eight times: one launch pair)
  world        Robot.set_world_depth of one frame, end to end from host arrays (copies, transform and installation)
  cloud        the route that exists without the map, on the same tensors: a torch back-projection of the image to a
               point cloud, then HipChain.occupancy_from_points.  It marks and carves nothing: the ratio next to it
               compares a call that also frees space and keeps evidence with one that does neither.

The floor is quoted from the bytes a call must move at the device's HBM rate (--hbm-gbs, 8000 by default: the MI355X's
peak): 4 bytes per node (the map read and written) plus 4 bytes per pixel written and read back by the gather."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from grid_cost import PANDA, once, stats, world_a  # noqa: E402
from optik_amd import Robot  # noqa: E402
from optik_amd.collision import DEPTH_DEFAULTS, MAP_UNKNOWN, spheres_along_chain, spheres_at  # noqa: E402
from optik_amd.device import HipChain  # noqa: E402

ORIGIN = [-1.28, -1.28, -1.28]
GRIDS = {"128": (0.02, (128, 128, 128)), "256": (0.01, (256, 256, 256))}
H, W = 480, 640
K = np.array([525.0, 525.0, 319.5, 239.5])
FAR = 10.0


def camera():
    """At (2.2, 0, 0.6), looking at the origin: x right, y down, z forward."""
    eye = np.array([2.2, 0.0, 0.6])
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def qrot(q, v):
    u = 2.0 * np.cross(q[:3], v)
    return v + q[3] * u + np.cross(q[:3], u)


def render(T, spheres, boxes):
    """z-depth of the spheres [M, 4] and oriented boxes [M, 10] (t, quaternion i j k w, half extents): one ray per
    pixel, p = eye + s * R (x, y, 1), so the parameter of the nearest hit is the z-depth."""
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(u - K[2]) / K[0], (v - K[3]) / K[1], np.ones((H, W))], axis=-1) @ T[:3, :3].T
    eye = T[:3, 3]
    depth = np.full((H, W), FAR)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in spheres:
            oc = eye - s[:3]
            a, b, c = (d * d).sum(-1), (d * oc).sum(-1), oc @ oc - s[3] * s[3]
            disc = b * b - a * c
            near = (-b - np.sqrt(np.maximum(disc, 0.0))) / a
            hit = (disc >= 0.0) & (near > 0.0) & (near < depth)
            depth = np.where(hit, near, depth)
        for bx in boxes:
            qc = np.array([-bx[3], -bx[4], -bx[5], bx[6]])
            e, dl = qrot(qc, eye - bx[:3]), qrot(qc, d)
            t0, t1 = (-bx[7:10] - e) / dl, (bx[7:10] - e) / dl
            near, far = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
            hit = (near <= far) & (near > 0.0) & (near < depth)
            depth = np.where(hit, near, depth)
    return depth.astype(np.float32)


def back_project(depth, T):
    """The cloud of an image on the device, in torch: what a caller of occupancy_from_points does today."""
    v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64, device="cuda"),
                          torch.arange(W, dtype=torch.float64, device="cuda"), indexing="ij")
    d = depth.to(torch.float64)
    d = torch.where((d > DEPTH_DEFAULTS["z_near"]) & (d <= DEPTH_DEFAULTS["z_far"]), d, torch.nan)
    pc = torch.stack([(u - K[2]) / K[0] * d, (v - K[3]) / K[1] * d, d], dim=-1).reshape(-1, 3)
    return (pc @ T[:3, :3].T + T[:3, 3]).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_cost.txt"))
    a = ap.parse_args()
    robot = Robot.from_urdf_file(*PANDA)
    frames, centers, radii = spheres_along_chain(robot, 0.05, 12)
    robot.set_collision_model(frames, centers, radii, self_pairs="auto", margin=0.0)
    hc = HipChain(**robot.chain_tables())
    lb, ub = (np.array(v) for v in robot.joint_limits())
    exclude = spheres_at(robot, 0.5 * (lb + ub), frames, centers, radii, pad=0.02)
    d_exclude = torch.tensor(exclude, dtype=torch.float64, device="cuda")
    T = camera()
    image = render(T, *world_a())
    d_one = torch.tensor(image, device="cuda")
    d_eight = d_one[None].repeat(8, 1, 1).contiguous()
    d_T = torch.tensor(T, device="cuda")
    T8 = np.stack([T] * 8)

    scenes = {}
    for name, (voxel, shape) in GRIDS.items():
        scenes[name] = dict(voxel=voxel, shape=shape,
                            map1=torch.full(shape, MAP_UNKNOWN, dtype=torch.int16, device="cuda"),
                            map8=torch.full(shape, MAP_UNKNOWN, dtype=torch.int16, device="cuda"),
                            host=Robot.new_depth_map(shape), into=torch.zeros(shape, dtype=torch.uint8, device="cuda"))

    def world(s):
        s["host"], _ = robot.set_world_depth(s["host"], ORIGIN, s["voxel"], image, K, T, exclude)

    calls = {
        "integrate1": lambda s: once(lambda: hc.depth_integrate(s["map1"], ORIGIN, s["voxel"], d_one, K, T, d_exclude)),
        "integrate8": lambda s: once(lambda: hc.depth_integrate(s["map8"], ORIGIN, s["voxel"], d_eight, K, T8, d_exclude)),
        "world": lambda s: once(lambda: world(s)),
        "cloud": lambda s: once(lambda: hc.occupancy_from_points(ORIGIN, s["voxel"], s["shape"], back_project(d_one, d_T),
                                                                 d_exclude, into=s["into"])),
    }
    times = {(g, c): [] for g in scenes for c in calls}
    for rep in range(a.reps + 1):  # (the first round warms up: workspace growth, first launches)
        for g, s in scenes.items():
            for c, fn in calls.items():
                dt, _ = fn(s)
                if rep:
                    times[(g, c)].append(dt)
    robot.clear_world_grid()

    lines = [f"# tools/depth_cost.py --reps {a.reps}: {H} x {W} depth image of section 5.12's scene "
             f"({int((image < FAR).sum())} surface pixels), {len(exclude)} exclusion spheres; wall-clock ms per call "
             "around a device synchronisation, interleaved in one process, median [min, max]",
             f"# device: {torch.cuda.get_device_name(0)}"]
    for g, s in scenes.items():
        nodes = int(np.prod(s["shape"]))
        seen = int((s["map1"] != MAP_UNKNOWN).sum())
        lines.append(f"grid {g}^3, voxel {s['voxel']}: {seen} of {nodes} nodes observed after the run")
        st = {c: stats(times[(g, c)]) for c in calls}
        for c in calls:
            lines.append(f"  {c:<11s} {st[c]['median_ms']:9.3f} ms  [{st[c]['min_ms']:.3f}, {st[c]['max_ms']:.3f}]")
        for c, F in (("integrate1", 1), ("integrate8", 8)):
            floor_ms = (4.0 * nodes + 8.0 * F * H * W) / (a.hbm_gbs * 1e9) * 1e3
            lines.append(f"  floor {c}: {floor_ms:.4f} ms at {a.hbm_gbs:.0f} GB/s (4 B per node + 8 B per pixel and "
                         f"frame); measured / floor = {st[c]['median_ms'] / floor_ms:.1f}")
        lines.append(f"  integrate8 / integrate1 = {st['integrate8']['median_ms'] / st['integrate1']['median_ms']:.2f}; "
                     f"integrate1 / cloud = {st['integrate1']['median_ms'] / st['cloud']['median_ms']:.2f} "
                     "(cloud = torch back-projection + occupancy_from_points: it carves nothing and keeps no evidence)")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
