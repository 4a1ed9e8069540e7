"""Test helper: the oracle of the device verifier.  tests/redetect_oracle.py with the PER-VIEW rule: one
fresh RigidRANSAC per view instead of one per getBestMatch call whose engine runs on from view to view.  Everything else --
the per-view match, views in ascending index, the first of equal errors, the decision block -- is redetect_oracle's."""
import numpy as np

import redetect_oracle as ro


def get_best_match(orc, query_desc, query_coord, views, config=ro.RANSAC_CONFIG):
    """redetect_oracle.get_best_match with one fresh RigidRANSAC per view"""
    from multimotionfusion_amd.ransac import RigidRANSAC
    best = dict(found=False, transformation=np.eye(4, dtype=np.float32), error=float("inf"), inliers=0, view=-1, n_matches=0,
                inlier=np.zeros(0, bool))
    if not views or len(query_desc) == 0:
        return best
    query_coord = np.ascontiguousarray(query_coord, np.float32)
    for v, ((desc, coord), (idx, _)) in enumerate(zip(views, ro.match_views(orc, query_desc, views))):
        if len(desc) == 0:
            continue
        sel = idx >= 0
        if int(sel.sum()) < 3:
            continue
        T, err, inl = RigidRANSAC(*config).estimate(query_coord[sel], np.asarray(coord, np.float32)[idx[sel]])
        if inl is None or int(inl.sum()) == 0:
            continue
        if not best["found"] or np.float32(err) < np.float32(best["error"]):
            best = dict(found=True, transformation=T, error=err, inliers=int(inl.sum()), view=v, n_matches=int(sel.sum()), inlier=inl)
    return best


def redetect(orc, *args, **kwargs):
    """redetect_oracle.redetect -- the decision block -- with the per-view getBestMatch"""
    saved = ro.get_best_match
    ro.get_best_match = get_best_match
    try:
        return ro.redetect(orc, *args, **kwargs)
    finally:
        ro.get_best_match = saved
