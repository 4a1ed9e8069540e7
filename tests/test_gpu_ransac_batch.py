"""-m gpu: RigidRANSAC for batches of independent problems on the device (csrc/ransac_kernels.hpp) against one fresh host
object per problem, bit for bit -- and, first, what that equality rests on: sqrt and division on doubles, sqrtf, float
division and rintf are correctly rounded on the device under the library's build flags."""
import ctypes as C

import numpy as np
import pytest
import torch

import ransac_cases as rc

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rounded_op(ctx, op, a, b, out_dtype):
    da, db = dev(a), (dev(b) if b is not None else None)
    out = torch.empty(a.size, dtype=out_dtype, device="cuda")
    from multimotionfusion_amd._capi import check
    check(ctx.lib.mmf_debug_rounded_ops(ctx.handle, op, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()) if db is not None else None,
                                        a.size, C.c_void_p(out.data_ptr())))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def doubles(rng, n):
    """random bit patterns (every exponent, denormals, infinities, NaNs) and the magnitudes the fits work at"""
    raw = rng.integers(0, 2 ** 64, n // 2, dtype=np.uint64).view(np.float64)
    near = (rng.normal(size=n - n // 2) * 10.0 ** rng.uniform(-12, 4, n - n // 2))
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 1e-300])
    return np.concatenate([raw, near, special])


def floats(rng, n):
    raw = rng.integers(0, 2 ** 32, n // 2, dtype=np.uint64).astype(np.uint32).view(np.float32)
    near = (rng.normal(size=n - n // 2) * 10.0 ** rng.uniform(-8, 4, n - n // 2)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1e-45, 1.17549435e-38, 3.4028235e38, 0.5, 1.5, 2.5, -0.5, -1.5, 8388607.5],
                       np.float32)
    return np.concatenate([raw, near, special])


def same(a, b):
    """bit-equal, every NaN equal to every NaN (the payload of an invalid operation's NaN is not part of IEEE 754 rounding)"""
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return ((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all()


def test_device_operations_are_correctly_rounded(gpu_ctx):
    """sqrt / division (double), sqrtf, float division, float / int and rintf on the device equal numpy's (IEEE 754
    correctly rounded, round to nearest even) bit for bit on more than 1 M arguments each."""
    rng = np.random.default_rng(2)
    n = 1 << 20
    with np.errstate(all="ignore"):
        a, b = doubles(rng, n), doubles(rng, n)
        assert same(rounded_op(gpu_ctx, 0, a, None, torch.float64), np.sqrt(a))
        assert same(rounded_op(gpu_ctx, 1, a, b, torch.float64), a / b)
        # the quotients the fit forms: sums over a count, a vector over its norm
        cnt = rng.integers(1, 1025, a.size).astype(np.float64)
        assert same(rounded_op(gpu_ctx, 1, a, cnt, torch.float64), a / cnt)
        x, y = floats(rng, n), floats(rng, n)
        assert same(rounded_op(gpu_ctx, 2, x, None, torch.float32), np.sqrt(x))
        assert same(rounded_op(gpu_ctx, 3, x, None, torch.float32), np.rint(x))
        assert same(rounded_op(gpu_ctx, 4, x, y, torch.float32), x / y)
        k = rng.integers(1, 1025, x.size).astype(np.int32)
        assert same(rounded_op(gpu_ctx, 5, x, k, torch.float32), x / k.astype(np.float32))
        halves = (np.arange(-70000, 70000, dtype=np.float32) + np.float32(0.5)) * np.float32(0.8)  # fraction * N near ties
        assert same(rounded_op(gpu_ctx, 3, halves, None, torch.float32), np.rint(halves))


@pytest.fixture(scope="module")
def ragged():
    """306 problems (sizes x kinds x 2) with n = 2 and n = max_points + 1 in their midst, and their per-problem host results"""
    from multimotionfusion_amd import ransac
    rng = np.random.default_rng(9)
    probs = rc.problems(2, seed=21)
    probs.insert(100, ("too_few", *rc.make("noise", 2, rng)))
    probs.insert(200, ("too_many", *rc.make("noise", 1025, rng)))
    ref = []
    for kind, p0, p1 in probs:
        ref.append(ransac.RigidRANSAC(*rc.CONFIG).estimate(p0, p1) if 3 <= len(p0) <= 1024 else None)
    return probs, ref


def check_batch(out, offsets, probs, ref):
    with_inliers = without = 0
    for k, ((kind, p0, p1), want) in enumerate(zip(probs, ref)):
        n = len(p0)
        flags = out["inlier"][offsets[k]:offsets[k + 1]]
        if want is None:
            assert out["status"][k] == (1 if n < 3 else 2), (k, n, out["status"][k])
            assert np.array_equal(out["T"][k], np.eye(4, dtype=np.float32)) and np.isposinf(out["error"][k])
            assert out["has_inlier"][k] == 0 and out["n_inliers"][k] == 0 and not flags.any()
            continue
        T, err, inl = want
        assert out["status"][k] == 0
        assert rc.same_bits(out["T"][k], T), (k, kind, n, out["T"][k], T)
        assert rc.same_bits(out["error"][k], np.float32(err)), (k, kind, n, out["error"][k], err)
        assert bool(out["has_inlier"][k]) == (inl is not None), (k, kind, n)
        if inl is None:
            without += 1
            assert out["n_inliers"][k] == 0 and not flags.any()
        else:
            with_inliers += 1
            assert np.array_equal(flags.astype(bool), inl) and out["n_inliers"][k] == inl.sum(), (k, kind, n)
    return with_inliers, without


def test_ragged_batch_equals_fresh_host_objects(gpu_ctx, ragged):
    from multimotionfusion_amd.ransac import RansacBatch
    probs, ref = ragged
    assert len(probs) >= 302
    offsets = np.concatenate([[0], np.cumsum([len(p[1]) for p in probs])]).astype(np.int32)
    p0 = dev(np.concatenate([p[1] for p in probs]))
    p1 = dev(np.concatenate([p[2] for p in probs]))
    b = RansacBatch(gpu_ctx, *rc.CONFIG, max_points=1024)
    out = b.estimate(p0, p1, offsets)
    assert b.last_launches() == 1
    with_inliers, without = check_batch(out, offsets, probs, ref)
    assert with_inliers > 50 and without > 50, (with_inliers, without)  # both outcomes occur
    again = b.estimate(p0, p1, offsets)  # the object keeps no state between calls
    assert all(np.array_equal(out[k].view(np.uint8), again[k].view(np.uint8)) for k in out)
    b.close()


@pytest.mark.parametrize("which", [4, 120, 290])
def test_batch_of_one(gpu_ctx, ragged, which):
    from multimotionfusion_amd.ransac import RansacBatch
    probs, ref = ragged
    _, p0, p1 = probs[which]
    b = RansacBatch(gpu_ctx, *rc.CONFIG, max_points=1024)
    offsets = np.array([0, len(p0)], np.int32)
    out = b.estimate(dev(p0), dev(p1), offsets)
    check_batch(out, offsets, [probs[which]], [ref[which]])
    empty = b.estimate(dev(p0[:0]), dev(p1[:0]), np.array([0], np.int32))
    assert empty["T"].shape == (0, 4, 4) and b.last_launches() == 0
    b.close()


def test_smaller_objects_and_other_configurations(gpu_ctx):
    """max_points below a wave and off a multiple of 64 (the LDS layout follows it), 1 and 32 iterations"""
    from multimotionfusion_amd import ransac
    rng = np.random.default_rng(33)
    for cfg, max_points in [((10, 0.03, 0.6), 40), ((1, 0.05, 0.5), 100), ((32, 0.01, 0.9), 3), ((32, 0.02, 0.3), 200)]:
        sizes = sorted({3, min(max_points, 17), max_points, max_points + 1, max(3, max_points // 2)})
        probs = [(k, *rc.make(k, n, rng)) for n in sizes for k in ("noise", "outliers30", "duplicates", "coplanar")]
        ref = [ransac.RigidRANSAC(*cfg).estimate(p0, p1) if len(p0) <= max_points else None for _, p0, p1 in probs]
        offsets = np.concatenate([[0], np.cumsum([len(p[1]) for p in probs])]).astype(np.int32)
        b = ransac.RansacBatch(gpu_ctx, *cfg, max_points=max_points)
        out = b.estimate(dev(np.concatenate([p[1] for p in probs])), dev(np.concatenate([p[2] for p in probs])), offsets)
        check_batch(out, offsets, probs, ref)
        b.close()


def test_create_and_estimate_refuse_bad_sizes(gpu_ctx):
    from multimotionfusion_amd._capi import MmfError
    from multimotionfusion_amd.ransac import RansacBatch
    for kw in (dict(max_points=2), dict(max_points=1025), dict(iterations=0), dict(iterations=33)):
        with pytest.raises(MmfError):
            RansacBatch(gpu_ctx, **kw)
    b = RansacBatch(gpu_ctx, max_points=64)
    p = dev(np.zeros((8, 3), np.float32))
    with pytest.raises(MmfError):
        b.estimate(p, p, np.array([0, 5, 3, 8], np.int32))  # descending
    b.close()
