"""-m gpu: mmf_tracker_backdate (csrc/backdate_kernels.hpp, csrc/backdate_host.hpp; Model::refineTrackSubset, Model.cpp:649-737)
against tests/backdate_oracle.py on the cases of tests/backdate_cases.py: every field of every entry, the rows handed to
the batch object and the launch count, bit for bit; twice the same bytes; the table and the log untouched."""
import numpy as np
import pytest
import torch

import backdate_cases as bc
import backdate_oracle as bo
import tracker_oracle as to

pytestmark = pytest.mark.gpu


class Driver:
    """the device tracker and the oracle, driven together"""

    def __init__(self, ctx, case):
        from multimotionfusion_amd.tracker import DevicePointTracker
        self.dev = DevicePointTracker(ctx, bc.W, bc.H, bc.K, capacity=case.capacity, max_keypoints=case.max_keypoints)
        self.ora = bo.BackdateOracle(to.OracleTracker(bc.W, bc.H, bc.K, capacity=case.capacity), 0)

    def log(self, frames):
        self.dev.setViewLog(frames)
        self.ora.set_view_log(frames)

    def add(self, xy, desc, ts, depth):
        self.dev.addKeypointsPixels(xy, desc, ts, torch.from_numpy(depth).cuda(), 0.7, 30)
        self.ora.add(xy, desc, ts, depth, 0.7, 30)

    def associate(self, mask, ids):
        self.dev.associate(torch.from_numpy(mask).cuda(), ids)
        self.ora.t.associate(mask, ids)

    def prune(self, min_kps, min_time):
        self.dev.prune(min_kps, min_time)
        self.ora.t.prune(min_kps, min_time)

    def reset(self):
        self.dev.reset()
        self.ora.reset()


@pytest.fixture(scope="module")
def batches(gpu_ctx):
    """one batch object per max_points the cases ask for, {10, 0.03, 0.6}: built once (the table takes a while at 1024)"""
    from multimotionfusion_amd.ransac import RansacBatch
    made = {}

    def get(max_points):
        if max_points not in made:
            made[max_points] = RansacBatch(gpu_ctx, *bo.CONFIG, max_points=max_points)
        return made[max_points]
    yield get
    for b in made.values():
        b.close()


def same_rows(got, want):
    return all(g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want))


@pytest.mark.parametrize("case", bc.cases(), ids=lambda c: c.name)
def test_every_case_matches_the_oracle_bit_for_bit(gpu_ctx, orc, batches, case):
    d = Driver(gpu_ctx, case)
    bc.replay(case, d)
    assert to.same_table(d.dev.download(), d.ora.t.flatten()) is None
    batch = batches(case.max_points)
    before, batch_before = d.dev.download(), batch.last_launches()
    got = d.dev.backdate(case.label, case.history, batch)
    assert d.dev.lastLaunches() == 3
    want, rows = d.ora.backdate(case.label, case.history, case.max_points)
    diff = bo.same_entries(got, want)
    assert diff is None, (case.name, diff)
    problems = sum(1 for j, e in enumerate(want) if j and e["status"] == bo.OK)
    assert batch.last_launches() == (1 if problems else batch_before)  # (without a problem the batch object is not called)
    for j in range(len(want)):
        assert same_rows(d.dev.backdateRows(j), rows[j]), (case.name, j)
    # a second run gives the same bytes, and neither wrote the table or the log
    again = d.dev.backdate(case.label, case.history, batch)
    assert bo.same_entries(again, got) is None
    for j in range(len(want)):
        assert same_rows(d.dev.backdateRows(j), rows[j]), (case.name, j)
    assert to.same_table(d.dev.download(), before) is None
    s = d.ora.stamp
    stamps = list(range(max(s - d.ora.frames, 0), s + 1))
    eye = [np.eye(4, dtype=np.float32)] * len(stamps)
    d.dev.associateAll([9])
    d.ora.t.associate_all([9])
    views, missing = d.dev.modelViews(9, stamps, eye)
    want_views, want_missing = d.ora.model_views(9, stamps, eye)
    assert missing == want_missing and bc.vo.same_views(views, want_views) is None
    d.dev.close()


def test_another_label_history_and_a_smaller_workspace_in_one_tracker(gpu_ctx, orc, batches):
    """one tracker, several calls: label 2 and label 0 of the same table, a history the workspace was not reserved for (it
    grows), then a smaller one (it stays); every call against the oracle"""
    case = next(c for c in bc.cases() if c.name == "other_labels")
    d = Driver(gpu_ctx, case)
    bc.replay(case, d)
    d.dev.reserveBackdate(2)
    batch = batches(1024)
    for label, history in ((2, 2), (0, 3), (1, 8), (7, 2), (1, 2)):
        got = d.dev.backdate(label, history, batch)
        want, rows = d.ora.backdate(label, history)
        assert bo.same_entries(got, want) is None, (label, history)
        assert d.dev.lastLaunches() == 3
        for j in range(len(want)):
            assert same_rows(d.dev.backdateRows(j), rows[j])
    d.dev.close()


def test_what_the_call_refuses(gpu_ctx, orc, batches):
    from multimotionfusion_amd._capi import MmfError, mmf_backdated_pose
    import ctypes as C
    case = next(c for c in bc.cases() if c.name == "history_3")
    d = Driver(gpu_ctx, case)
    bc.replay(case, d)
    batch = batches(1024)
    lib, n = gpu_ctx.lib, C.c_int()
    out = (mmf_backdated_pose * 4)()
    assert lib.mmf_tracker_backdate(d.dev.handle, 1, 3, batch.handle, out, 2, C.byref(n)) == -1  # capacity 2 < 3 entries
    assert lib.mmf_tracker_backdate(d.dev.handle, 1, 1, batch.handle, out, 4, C.byref(n)) == -1  # history < 2
    assert lib.mmf_tracker_backdate(d.dev.handle, 1, 257, batch.handle, out, 4, C.byref(n)) == -1  # above the cap
    assert lib.mmf_tracker_backdate(d.dev.handle, 256, 3, batch.handle, out, 4, C.byref(n)) == -1  # no such label
    assert lib.mmf_tracker_backdate(d.dev.handle, 1, 3, None, out, 4, C.byref(n)) == -1
    assert lib.mmf_tracker_backdate(d.dev.handle, 1, 3, batch.handle, out, 3, C.byref(n)) == 0 and n.value == 3
    from multimotionfusion_amd.cudafuncs import Context
    from multimotionfusion_amd.ransac import RansacBatch
    other = Context(0, use_torch_stream=False)
    try:
        foreign = RansacBatch(other, *bo.CONFIG, max_points=8)
        assert lib.mmf_tracker_backdate(d.dev.handle, 1, 3, foreign.handle, out, 4, C.byref(n)) == -1  # another context's
        assert b"context" in lib.mmf_last_error()
        foreign.close()
    finally:
        other.close()
    d.dev.setViewLog(0)
    assert lib.mmf_tracker_backdate(d.dev.handle, 1, 3, batch.handle, out, 4, C.byref(n)) == -4  # no log: MMF_ERR_STATE
    with pytest.raises(MmfError):
        d.dev.backdateRows(0)  # (the log changed: the last call's rows are gone)
    d.dev.close()
