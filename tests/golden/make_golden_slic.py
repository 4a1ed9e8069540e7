"""Generates tests/golden/slic_engine_*.npz from tests/slic_oracle.py: synthetic frames, the label image and the centres
and counts after every iteration.  gSLICr is not in the reference tree and cannot run here, so these pin the ORACLE's
restatement of the specification, not the library ("parity unpinned").
Re-run: python tests/golden/make_golden_slic.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import slic_oracle as so  # noqa: E402
from multimotionfusion_amd import synth  # noqa: E402

for w, h, S, seed in [(160, 120, 20, 3), (320, 240, 16, 5)]:
    pose = synth.trajectory(2, seed=21)[1]
    objs = synth.make_objects(1, seed=21)
    traj = synth.object_trajectories(objs, 2, seed=21, trans_mm=60.0, rot_deg=2.0)
    rgb = synth.render(pose, w, h, seed=seed, objects=objs, object_poses=[t[1] for t in traj])["rgb"]
    trace = []
    labels, centres, counts = so.segment(rgb, S, 5, trace=trace)
    assert labels.max() < 32768
    np.savez_compressed(os.path.join(HERE, f"slic_engine_{w}x{h}_s{S}.npz"), rgb=rgb, spixel_size=np.int32(S),
                        labels=labels.astype(np.int16), labels_first=trace[0][0].astype(np.int16),
                        centres_iter=np.stack([t[1] for t in trace]), counts_iter=np.stack([t[2] for t in trace]),
                        centres=centres, counts=counts)
