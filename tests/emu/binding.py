"""ctypes binding of the host emulation of the tuned solvers (tests/emu/quad_emu.cpp) and of the general solver of
the 9 .. 16 joint chains (tests/emu/wide_emu.cpp).

Test infrastructure: built with the ROCm clang as plain host C++ (-ffp-contract=off), the device
headers of optik_amd/csrc compiled under OPTIK_LANE_EMU.  Nothing in the product imports this."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "optik_amd", "csrc")
LIB = os.path.join(HERE, "libquad_emu.so")
SRC = os.path.join(HERE, "quad_emu.cpp")
WIDE_SRC = os.path.join(HERE, "wide_emu.cpp")
WIDE_LIB = os.path.join(HERE, "libwide_emu.so")
WIDE_LIB_GENERAL_LSI = os.path.join(HERE, "libwide_emu_general_lsi.so")  # the same source, -DOPTIK_WIDE_GENERAL_LSI
WIDE_FORMS = {"WPG": 0, "WPL": 1, "WPC": 2}
_lib = None
_wide_libs = {}


def _clang():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("amdclang++"), shutil.which("clang++")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("no clang++ found (the emulation needs ext_vector_type)")


def build(force=False):
    deps = [SRC, os.path.join(HERE, "lane_emu.hpp")] + [
        os.path.join(CSRC, h) for h in ("ik_quad.hpp", "ik_lane64.hpp", "ik_lane.hpp", "ik_platform.hpp", "ik_math.hpp", "ik_eval.hpp", "ik_slsqp.hpp",
                                        "ik_solve.hpp", "ik_nnls_quad.hpp", "ik_nnls_first.hpp", "ik_host_params.hpp")]
    if not force and os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    subprocess.check_call([_clang(), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread",
                           "-I", HERE, "-I", CSRC, "-Wno-unused-value", "-Wno-psabi",
                           # (the emulated waves are a few lanes wide: the per-lane first NNLS pass of ik_nnls_first.hpp, which the
                           # device only runs on trips with more than 24 problems, runs on every trip here)
                           "-DOPTIK_LANE_FIRST_PASS_MIN=0", *os.environ.get("OPTIK_EMU_EXTRA_FLAGS", "").split(), SRC, "-o", LIB])
    return LIB


def lib():
    global _lib
    if _lib is None:
        from optik_amd import _native as nat
        L = C.CDLL(build())
        dp = C.POINTER(C.c_double)
        ip = C.POINTER(C.c_int32)
        L.quad_emu_solve.argtypes = [dp, dp, C.c_int, C.c_int, dp, dp, C.POINTER(nat.SolverConfigC), dp, dp, dp,
                                     C.c_uint64, C.c_uint64, C.c_int, C.c_int, dp, dp, dp, ip, ip, C.c_int]
        _lib = L
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def solve(chain, cfg, target7, x0, begin, end, quads=1, range_rule=0, ee_offset7=None, lane64=False):
    """chain: dict(types, origins[J,7], axes[J,3], lb, ub).  Returns dict(x[R,n], f, key, status, evals)."""
    origins = np.ascontiguousarray(chain["origins"], dtype=np.float64)
    n = len(chain["lb"])
    axes = np.ascontiguousarray(np.asarray(chain["axes"], dtype=np.float64)[:n])
    lb, ub = (np.ascontiguousarray(chain[k], dtype=np.float64) for k in ("lb", "ub"))
    tg = np.ascontiguousarray(target7, dtype=np.float64)
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
    R = end - begin
    out_x = np.zeros((n, R))
    out_f, out_key = np.zeros(R), np.zeros(R)
    status, evals = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    rc = lib().quad_emu_solve(_dp(origins), _dp(axes), n, origins.shape[0], _dp(lb), _dp(ub), C.byref(cfg), _dp(tg),
                              _dp(x0), _dp(ee) if ee is not None else None, begin, end, quads, range_rule,
                              _dp(out_x), _dp(out_f), _dp(out_key), status.ctypes.data_as(C.POINTER(C.c_int32)),
                              evals.ctypes.data_as(C.POINTER(C.c_int32)), 1 if lane64 else 0)
    if rc:
        raise RuntimeError(f"quad_emu_solve rc={rc}")
    return dict(x=out_x.T.copy(), f=out_f, key=out_key, status=status, evals=evals)


# ---- the general solver (ik_wide.hpp) ---------------------------------------------------------------------------

def _wide_flags():
    return ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", HERE, "-I", CSRC,
            "-Wno-unused-value", "-Wno-psabi"]


def build_wide(general_lsi=False, force=False, src=None, out=None, include_first=None):
    """libwide_emu.so, or with general_lsi the -DOPTIK_WIDE_GENERAL_LSI build of the same source.  src / out /
    include_first: another copy of the source, another library file, a directory searched before optik_amd/csrc (a
    test that builds the emulation from an edited copy of a device header)."""
    src = src or WIDE_SRC
    out = out or (WIDE_LIB_GENERAL_LSI if general_lsi else WIDE_LIB)
    deps = [src, os.path.join(HERE, "lane_emu.hpp")] + [
        os.path.join(CSRC, h) for h in ("ik_wide.hpp", "ik_wide_launch.hpp", "ik_jacobian.hpp", "ik_launch.hpp", "ik_platform.hpp",
                                        "ik_math.hpp", "ik_eval.hpp", "ik_slsqp.hpp", "ik_solve.hpp", "ik_host_params.hpp")]
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in deps):
        return out
    flags = _wide_flags()
    if include_first:
        flags = flags[:6] + ["-I", include_first] + flags[6:]
    subprocess.check_call([_clang(), *flags, *(["-DOPTIK_WIDE_GENERAL_LSI"] if general_lsi else []), src, "-o", out])
    return out


def wide_lib(path=None, general_lsi=False):
    path = path or build_wide(general_lsi)
    if path not in _wide_libs:
        from optik_amd import _native as nat
        L = C.CDLL(path)
        dp = C.POINTER(C.c_double)
        ip = C.POINTER(C.c_int32)
        cfgp = C.POINTER(nat.SolverConfigC)
        L.wide_emu_solve.argtypes = [dp, dp, C.c_int, C.c_int, dp, dp, cfgp, dp, dp, dp, C.c_uint64, C.c_uint64,
                                     C.c_int, C.c_int, C.c_int, dp, dp, dp, ip, ip]
        L.wide_emu_ops.argtypes = [dp, dp, C.c_int, C.c_int, dp, dp, cfgp, dp, dp, C.c_int, dp, C.c_longlong, dp, dp,
                                   dp, dp, C.c_uint64, C.c_longlong, dp]
        _wide_libs[path] = L
    return _wide_libs[path]


def _chain_arrays(chain):
    origins = np.ascontiguousarray(chain["origins"], dtype=np.float64)
    n = len(chain["lb"])
    axes = np.ascontiguousarray(np.asarray(chain["axes"], dtype=np.float64)[:n])
    lb, ub = (np.ascontiguousarray(chain[k], dtype=np.float64) for k in ("lb", "ub"))
    return origins, axes, n, lb, ub


def wide_solve(chain, cfg, target7, x0, begin, end, form="WPG", lanes=4, range_rule=0, ee_offset7=None, lib_path=None,
               general_lsi=False):
    """wide_solve_wave in one of its forms ("WPG" on `lanes` lanes, "WPL", "WPC"): dict(x[R,n], f, key, status, evals)."""
    origins, axes, n, lb, ub = _chain_arrays(chain)
    tg = np.ascontiguousarray(target7, dtype=np.float64)
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
    R = end - begin
    out_x = np.zeros((n, R))
    out_f, out_key = np.zeros(R), np.zeros(R)
    status, evals = np.zeros(R, dtype=np.int32), np.zeros(R, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    rc = wide_lib(lib_path, general_lsi).wide_emu_solve(
        _dp(origins), _dp(axes), n, origins.shape[0], _dp(lb), _dp(ub), C.byref(cfg), _dp(tg), _dp(x0),
        _dp(ee) if ee is not None else None, begin, end, WIDE_FORMS[form], lanes, range_rule, _dp(out_x), _dp(out_f),
        _dp(out_key), status.ctypes.data_as(ip), evals.ctypes.data_as(ip))
    if rc:
        raise RuntimeError(f"wide_emu_solve rc={rc}")
    return dict(x=out_x.T.copy(), f=out_f, key=out_key, status=status, evals=evals)


def wide_ops(chain, cfg, target7=None, q=None, ee_offset7=None, seeds=None, range_rule=0, jacobian=True):
    """wide_eval_fg (f [B], g [B,n]; with target7), wide_forward + wide_jacobian_column (pose [B,7], jac [B,6n]) at the
    rows of q, and wide_restart_seed for seeds = (first index, count) (seeds [count,n])."""
    origins, axes, n, lb, ub = _chain_arrays(chain)
    out = {}
    null = None
    B = 0
    qa = None
    if q is not None:
        qa = np.ascontiguousarray(q, dtype=np.float64)
        B = qa.shape[0]
        out["pose"] = np.zeros((B, 7))
        if jacobian:
            out["jac"] = np.zeros((B, 6 * n))
        if target7 is not None:
            out["f"], out["g"] = np.zeros(B), np.zeros((B, n))
    tg = np.ascontiguousarray(target7 if target7 is not None else [0, 0, 0, 0, 0, 0, 1.0], dtype=np.float64)
    ee = np.ascontiguousarray(ee_offset7, dtype=np.float64) if ee_offset7 is not None else None
    first, count = seeds if seeds is not None else (0, 0)
    if count:
        out["seeds"] = np.zeros((count, n))
    ptr = lambda k: _dp(out[k]) if k in out else null  # noqa: E731
    rc = wide_lib().wide_emu_ops(_dp(origins), _dp(axes), n, origins.shape[0], _dp(lb), _dp(ub), C.byref(cfg), _dp(tg),
                                 _dp(ee) if ee is not None else None, range_rule, _dp(qa) if qa is not None else null,
                                 B, ptr("f"), ptr("g"), ptr("pose"), ptr("jac"), first, count, ptr("seeds"))
    if rc:
        raise RuntimeError(f"wide_emu_ops rc={rc}")
    return out
