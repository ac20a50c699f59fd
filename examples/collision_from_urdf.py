"""A collision model straight from a URDF's <collision> geometry: spheres fitted on the GPU to every link's boxes,
cylinders and STL meshes (Robot.set_collision_model_from_urdf), then collision-free IK
against an obstacle with it.

    python examples/collision_from_urdf.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from optik_amd import Robot, SolverConfig  # noqa: E402
from mesh_util import box_triangles, write_stl_binary  # noqa: E402

URDF = os.path.join(ROOT, "tests", "golden", "robots", "arm_primitives.urdf")


def main():
    # the one mesh the model names (package://arm_description/meshes/wedge.stl), written where mesh_dir points
    mesh_dir = tempfile.mkdtemp(prefix="arm_description_")
    os.makedirs(os.path.join(mesh_dir, "meshes"))
    write_stl_binary(os.path.join(mesh_dir, "meshes", "wedge.stl"), box_triangles([0.0, -0.06, -0.06], [0.2, 0.06, 0.06]))

    robot = Robot.from_urdf_file(URDF, "base", "tip")
    frames, centers, radii, report = robot.set_collision_model_from_urdf(URDF, "base", "tip", per_link=16,
                                                                         mesh_dir=mesh_dir)
    print(f"{len(radii)} spheres on frames {sorted(set(frames.tolist()))}; per frame {report['spheres_per_frame']}")
    print(f"surface samples left uncovered: {report['uncovered']} (0: the model contains the geometry)")
    for f, info in report["fits"].items():
        print(f"  frame {f}: grid {info['shape']}, {info['points']} samples, pad {info['pad']:.4f} m")
    print("skipped:", [s["link"] for s in report["geometry"]["skipped"]])
    print(f"self pairs kept {len(report['pairs'])}, dropped as always overlapping {len(report['pairs_dropped'])}")

    # an obstacle next to the arm, and IK that avoids it
    robot.set_world(spheres=[[0.25, 0.15, 0.55, 0.08]])
    x_goal = np.array([0.6, 0.4, -0.5])
    target = robot.fk(x_goal)
    sol = robot.ik(SolverConfig("quality", max_time=0.0, max_restarts=256), target, np.zeros(3))
    if sol is None:
        print("no collision-free solution")
    else:
        print("q =", np.round(sol[0], 4).tolist(), " clearance =", round(robot.collision_clearance(sol[0]), 4))


if __name__ == "__main__":
    main()
