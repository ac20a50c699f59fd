"""optik_amd/csrc/depth_measure.hpp compiled with g++ as plain C++ (no HIP runtime) for the host and the -m gpu tests of
depth-image worlds; an independent vectorised numpy restatement of its steps 1 - 4 in the same operation order; and the
scenes both tests share.

Every file the driver reads or writes holds doubles; int16, bytes and float32 values travel as doubles (exact both
ways, NaN and the infinities included)."""
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "optik_amd", "csrc")
UNKNOWN = -32768

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "depth_measure.hpp"

using namespace optik;

static std::vector<double> read_all(const char *path) {
    std::vector<double> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) return v;
    double x;
    while (std::fread(&x, sizeof(double), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    const std::vector<double> in = read_all(argv[2]);
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    if (argv[1][0] == 'i') {
        // origin (3), voxel, nx, ny, nz, F, H, W, E, z_near, z_far, band, hit, miss, e_min, e_max, then map [nodes],
        // depth [F][H][W], intrinsics [F][4], poses [F][16], exclude [E][4] -> map [nodes]
        const double *origin = &in[0], voxel = in[3];
        const int32_t n[3] = {(int32_t)in[4], (int32_t)in[5], (int32_t)in[6]};
        const int F = (int)in[7], H = (int)in[8], W = (int)in[9], E = (int)in[10];
        depth::Params P;
        P.z_near = in[11]; P.z_far = in[12]; P.band = in[13];
        P.hit = (int32_t)in[14]; P.miss = (int32_t)in[15]; P.e_min = (int32_t)in[16]; P.e_max = (int32_t)in[17];
        const size_t nodes = (size_t)n[0] * n[1] * n[2], pixels = (size_t)F * H * W;
        if (in.size() != 18 + nodes + pixels + 20 * (size_t)F + 4 * (size_t)E) return 2;
        const double *p = &in[18];
        std::vector<int16_t> map(nodes);
        for (size_t i = 0; i < nodes; ++i) map[i] = (int16_t)p[i];
        p += nodes;
        std::vector<float> img(pixels), cleaned((size_t)H * W);
        for (size_t i = 0; i < pixels; ++i) img[i] = (float)p[i];
        p += pixels;
        depth::integrate(origin, voxel, n, map.data(), img.data(), F, H, W, p, p + 4 * (size_t)F, p + 20 * (size_t)F, E, P,
                         cleaned.data());
        for (size_t i = 0; i < nodes; ++i) {
            const double d = (double)map[i];
            std::fwrite(&d, sizeof(double), 1, out);
        }
    } else {
        // nodes, threshold, unknown_occupied, accumulate, then map [nodes], occupied [nodes] -> occupied [nodes]
        const size_t nodes = (size_t)in[0];
        if (in.size() != 4 + 2 * nodes) return 2;
        std::vector<int16_t> map(nodes);
        std::vector<uint8_t> occ(nodes);
        for (size_t i = 0; i < nodes; ++i) { map[i] = (int16_t)in[4 + i]; occ[i] = (uint8_t)in[4 + nodes + i]; }
        depth::occupancy_from_map(map.data(), (long long)nodes, (int)in[1], in[2] != 0.0, in[3] != 0.0, occ.data());
        for (size_t i = 0; i < nodes; ++i) {
            const double d = (double)occ[i];
            std::fwrite(&d, sizeof(double), 1, out);
        }
    }
    std::fclose(out);
    return 0;
}
"""

# the parameters the shared cases run with (not the library's defaults: a test pins its own)
PARAMS = dict(z_near=0.1, z_far=0.8, band=0.05, hit=3, miss=2, e_min=-7, e_max=11)


def _cams(intrinsics, poses, F):
    k = np.asarray(intrinsics, dtype=np.float64)
    k = np.broadcast_to(k, (F, 4)) if k.shape == (4,) else k
    p = np.asarray(poses, dtype=np.float64)
    p = p[None] if p.shape == (4, 4) else p
    assert k.shape == (F, 4) and p.shape == (F, 4, 4)
    return k, p


def _stack(depth):
    d = np.asarray(depth, dtype=np.float32)
    return d[None] if d.ndim == 2 else d


def build_depth_ref(workdir=None):
    """Compile the driver; returns an object with
    .integrate(map int16 [nx, ny, nz], origin, voxel, depth [F, H, W] or [H, W], intrinsics, poses (row-major 4x4),
               exclude=None, **params) -> int16 [nx, ny, nz] and
    .occupancy(map, threshold, unknown_occupied=False, into=None) -> uint8 [nx, ny, nz]."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler (g++) is needed to compile the depth header on its own"
    d = workdir or tempfile.mkdtemp(prefix="depth_measure_")
    src, exe = os.path.join(d, "depth_driver.cpp"), os.path.join(d, "depth_driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    # the library's numerical contract: no contraction into FMAs (optik_amd/build.py)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe],
                   check=True)

    def run(mode, parts):
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts]).tofile(fin)
        subprocess.run([exe, mode, fin, fout], check=True)
        return np.fromfile(fout, dtype=np.float64)

    class Ref:
        @staticmethod
        def integrate(map, origin, voxel, depth, intrinsics, poses, exclude=None, **params):
            P = dict(PARAMS, **params)
            map = np.asarray(map, dtype=np.int16)
            img = _stack(depth)
            F, H, W = img.shape
            k, p = _cams(intrinsics, poses, F)
            exc = np.zeros((0, 4)) if exclude is None else np.asarray(exclude, dtype=np.float64).reshape(-1, 4)
            head = [*np.asarray(origin, dtype=np.float64), float(voxel), *map.shape, F, H, W, len(exc), P["z_near"],
                    P["z_far"], P["band"], P["hit"], P["miss"], P["e_min"], P["e_max"]]
            out = run("i", [head, map, img, k, p.transpose(0, 2, 1), exc])  # (column-major poses, as the C ABI takes them)
            assert out.shape == (map.size,)
            return out.astype(np.int16).reshape(map.shape)

        @staticmethod
        def occupancy(map, threshold, unknown_occupied=False, into=None):
            map = np.asarray(map, dtype=np.int16)
            occ = np.zeros(map.shape, dtype=np.uint8) if into is None else np.asarray(into, dtype=np.uint8)
            out = run("o", [[map.size, threshold, float(bool(unknown_occupied)), float(into is not None)], map, occ])
            return out.astype(np.uint8).reshape(map.shape)

    return Ref()


# ---- the same steps in numpy: written from the contract, vectorised over pixels and over nodes ------------------------

def np_clean(img, K, T, exclude, z_near, z_far):
    """Step 1 for one frame: float32 [H, W].  K = (fx, fy, cx, cy), T = the camera's row-major 4x4."""
    fx, fy, cx, cy = (np.float64(x) for x in K)
    R, t = T[:3, :3], T[:3, 3]
    H, W = img.shape
    d = img.astype(np.float64)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        invalid = ~np.isfinite(d) | ~(d > z_near)
        far = ~invalid & (d > z_far)
        xc = ((u - cx) / fx) * d
        yc = ((v - cy) / fy) * d
        p = [((R[a, 0] * xc + R[a, 1] * yc) + R[a, 2] * d) + t[a] for a in range(3)]
        masked = np.zeros((H, W), dtype=bool)
        for s in (np.zeros((0, 4)) if exclude is None else np.asarray(exclude, dtype=np.float64).reshape(-1, 4)):
            dx, dy, dz = p[0] - s[0], p[1] - s[1], p[2] - s[2]
            masked |= ((dx * dx + dy * dy) + dz * dz) <= s[3] * s[3]
    out = np.where(masked, -img, img).astype(np.float32)
    out[far] = np.inf
    out[invalid] = np.nan
    return out


def np_integrate(map, origin, voxel, depth, intrinsics, poses, exclude=None, **params):
    """Steps 1 - 3: the map after the frames of `depth`, int16 [nx, ny, nz]."""
    P = dict(PARAMS, **params)
    img = _stack(depth)
    k, poses = _cams(intrinsics, poses, len(img))
    e = np.asarray(map, dtype=np.int16).astype(np.int32)
    origin, voxel = np.asarray(origin, dtype=np.float64), np.float64(voxel)
    ii, jj, kk = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in e.shape), indexing="ij")
    px, py, pz = origin[0] + voxel * ii, origin[1] + voxel * jj, origin[2] + voxel * kk
    for f in range(len(img)):
        fx, fy, cx, cy = (np.float64(x) for x in k[f])
        R, t = poses[f][:3, :3], poses[f][:3, 3]
        H, W = img[f].shape
        c = np_clean(img[f], k[f], poses[f], exclude, P["z_near"], P["z_far"])
        q0, q1, q2 = px - t[0], py - t[1], pz - t[2]
        xc = (R[0, 0] * q0 + R[1, 0] * q1) + R[2, 0] * q2
        yc = (R[0, 1] * q0 + R[1, 1] * q1) + R[2, 1] * q2
        zc = (R[0, 2] * q0 + R[1, 2] * q1) + R[2, 2] * q2
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ok = (zc > P["z_near"]) & (zc <= P["z_far"])
            wu = (fx * (xc / zc) + cx) + 0.5
            wv = (fy * (yc / zc) + cy) + 0.5
            ok &= (wu >= 0.0) & (wu < np.float64(W)) & (wv >= 0.0) & (wv < np.float64(H))
            col = np.where(ok, np.floor(wu), 0.0).astype(np.int64)
            row = np.where(ok, np.floor(wv), 0.0).astype(np.int64)
            cv = c[row, col]
            a = np.abs(cv.astype(np.float64))
            ok &= ~np.isnan(cv)
            miss = ok & (zc < a - P["band"])
            hit = ok & ~miss & (cv > 0) & np.isfinite(a) & (zc <= a + P["band"])
        base = np.where(e == UNKNOWN, 0, e)
        e = np.where(miss, np.maximum(base - P["miss"], P["e_min"]), np.where(hit, np.minimum(base + P["hit"], P["e_max"]), e))
    return e.astype(np.int16)


def np_occupancy(map, threshold, unknown_occupied=False, into=None):
    map = np.asarray(map, dtype=np.int16)
    occ = np.where(map == UNKNOWN, bool(unknown_occupied), map >= threshold).astype(np.uint8)
    return occ if into is None else (np.asarray(into, dtype=np.uint8) | occ)


# ---- the scenes the host test and the -m gpu test share -------------------------------------------------------------
SHAPE, VOXEL = (12, 10, 9), 0.05           # 1080 nodes: 16 waves and a partial one
ORIGIN = np.array([-0.3, -0.25, 0.125])     # the grid spans x -0.3 .. 0.25, y -0.25 .. 0.2, z 0.125 .. 0.525
IMG = (24, 32)                              # H, W: 768 pixels
K = np.array([20.0, 20.0, 15.5, 11.5])      # fx, fy, cx, cy: the grid's near face fills most of the image
WALL = 0.4                                  # a fronto-parallel wall for the identity camera: z = 0.4


def new_map(shape=SHAPE):
    return np.full(shape, UNKNOWN, dtype=np.int16)


def node_positions(origin=ORIGIN, voxel=VOXEL, shape=SHAPE):
    ii, jj, kk = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing="ij")
    return np.stack([origin[0] + voxel * ii, origin[1] + voxel * jj, origin[2] + voxel * kk], axis=-1)


def rot(axis, angle):
    c, s = math.cos(angle), math.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def pose(R=None, t=(0.0, 0.0, 0.0)):
    T = np.eye(4)
    T[:3, :3] = np.eye(3) if R is None else R
    T[:3, 3] = t
    return T


def tilted_pose():
    """Rotated about two axes and translated: the camera looks into the grid from a corner behind it, so some nodes are
    behind it, some outside the image and some beyond z_far."""
    return pose(rot(1, 0.45) @ rot(0, -0.3), (-0.35, 0.05, 0.2))


def wall_image(value=WALL):
    return np.full(IMG, value, dtype=np.float32)


def invalid_image():
    """The wall, with one column block each of NaN, 0, a negative value, +inf, a value below z_near and one above
    z_far (PARAMS: 0.1, 0.8)."""
    img = wall_image()
    bad = [np.nan, 0.0, -0.4, np.inf, 0.05, 2.0]
    for b, val in enumerate(bad):
        img[:, 4 * b + 2:4 * b + 6] = val
    return img, bad


def random_image(seed, lo=0.15, hi=0.7):
    rng = np.random.default_rng(seed)
    img = rng.uniform(lo, hi, IMG).astype(np.float32)
    img[rng.random(IMG) < 0.05] = np.nan
    img[rng.random(IMG) < 0.05] = 3.0
    return img


def cases():
    """[(name, dict(map, depth, intrinsics, poses, exclude, params))]: what the serial reference is compared on with the
    numpy twin and the device with the serial reference.  Deterministic."""
    rng = np.random.default_rng(23)
    seen = rng.integers(-7, 12, SHAPE).astype(np.int16)
    seen[rng.random(SHAPE) < 0.3] = UNKNOWN
    inval, _ = invalid_image()
    sphere = np.array([[0.0, 0.0, WALL, 0.12], [0.2, 0.1, 0.3, 0.05], [math.nan, 0.0, 0.4, 1.0]])
    three = np.stack([random_image(5), wall_image(), random_image(6)])
    three_poses = np.stack([tilted_pose(), pose(), pose(rot(2, 0.2), (0.02, -0.03, 0.0))])
    three_k = np.stack([K, K * [1.1, 0.9, 1.0, 1.0], K + [0.0, 0.0, 0.25, -0.5]])
    return [
        ("wall", dict(map=new_map(), depth=wall_image(), intrinsics=K, poses=pose(), exclude=None, params={})),
        ("invalid", dict(map=new_map(), depth=inval, intrinsics=K, poses=pose(), exclude=None, params={})),
        ("tilted", dict(map=seen, depth=random_image(7), intrinsics=K, poses=tilted_pose(), exclude=None,
                        params=dict(z_far=0.45))),
        ("selffilter", dict(map=new_map(), depth=wall_image(), intrinsics=K, poses=pose(), exclude=sphere, params={})),
        ("band0", dict(map=seen, depth=random_image(8), intrinsics=K, poses=pose(), exclude=sphere,
                       params=dict(band=0.0, hit=1024, miss=1024, e_min=-32767, e_max=32767))),
        ("frames3", dict(map=seen, depth=three, intrinsics=three_k, poses=three_poses, exclude=sphere, params={})),
    ]
