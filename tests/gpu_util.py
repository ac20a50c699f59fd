"""Helpers shared by the -m gpu parity tests (HIP path vs CPU oracle)."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bit_equal(got, want, what=""):
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    # +0.0 == -0.0 and NaN == NaN count as equal: only the sign of an exact zero may
    # differ (the kernels skip multiplications by structural zeros, see ik_slsqp.hpp)
    same = (bits(got) == bits(want)) | ((got == 0.0) & (want == 0.0)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        bad = np.argwhere(~same)
        i = tuple(bad[0])
        raise AssertionError(
            f"{what}: {len(bad)} of {got.size} values differ; first at {i}: "
            f"gpu={got[i]!r} oracle={want[i]!r} (diff {got[i] - want[i]:.3e})")


# Output buffers filled with a sentinel right before a call -- a NaN with a payload of its own for float64 and float32,
# 0x7f bytes for integers and flags --, none of which may remain: a kernel that skips an element cannot pass on what
# the caching allocator left in the block.
F64_SENTINEL, F32_SENTINEL, BYTE_SENTINEL = 0x7FF8000000005E17, 0x7FC05E17, 0x7F


def _out(shape, dtype):
    import torch
    t = torch.empty(shape, dtype=dtype, device="cuda")
    if dtype == torch.float64:
        t.view(torch.int64).fill_(F64_SENTINEL)
    elif dtype == torch.float32:
        t.view(torch.int32).fill_(F32_SENTINEL)
    else:
        t.view(torch.uint8).fill_(BYTE_SENTINEL)
    return t


def _sentinels_left(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return int((a.view(np.uint64) == F64_SENTINEL).sum())
    if a.dtype == np.float32:
        return int((a.view(np.uint32) == F32_SENTINEL).sum())
    return int((a.view(np.uint8).reshape(a.shape + (a.itemsize,)) == BYTE_SENTINEL).all(axis=-1).sum())


def make_targets(oracle, chain_dict, ch, rng, T):
    """Reachable targets FK(q*) and in-limit seeds, as examples/example.rs:24-26."""
    tg, x0 = [], []
    for _ in range(T):
        qt = rng.uniform(chain_dict["lb"], chain_dict["ub"])
        _, ee = oracle.fk(ch, qt)
        tg.append(ee)
        x0.append(rng.uniform(chain_dict["lb"], chain_dict["ub"]))
    return np.array(tg), np.array(x0)
