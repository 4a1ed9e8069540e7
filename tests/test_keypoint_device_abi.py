"""CPU: the exports of the keypoint path that stays on the device (include/mmf_hip.h: mmf_superpoint_get_features_device and
its neighbours, mmf_tracker_add_keypoints_device, mmf_fusion_set_keypoint_frontend) -- present in the library, bound in the
ctypes table, with the defaults the reference's processFrame uses, and refusing what they can refuse without a device."""
import ctypes as C

NEW = ["mmf_superpoint_get_features_device", "mmf_superpoint_device_features", "mmf_superpoint_device_status",
       "mmf_superpoint_last_features",
       "mmf_superpoint_last_launches", "mmf_tracker_add_keypoints_device", "mmf_tracker_set_keypoint_status",
       "mmf_tracker_keypoint_failures", "mmf_keypoint_frontend_default_config", "mmf_fusion_set_keypoint_frontend"]


def test_exports_are_bound_and_the_abi_version_stays():
    from multimotionfusion_amd import _capi
    lib = _capi.load()
    for name in NEW:
        assert name in _capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == _capi.SIGNATURES[name][1], name
    assert lib.mmf_abi_version() == 3


def test_default_config_is_the_references():
    """MultiMotionFusion.cpp:240-246: addKeypoints(..., 0.7f, 30), prune(30, t - 1 s); SuperPoint's 0.015 / 4 / 4"""
    from multimotionfusion_amd import _capi
    lib = _capi.load()
    cfg = _capi.mmf_keypoint_frontend_config()
    assert lib.mmf_keypoint_frontend_default_config(C.byref(cfg)) == 0
    assert cfg.conf_thresh == C.c_float(0.015).value and (cfg.nms_dist, cfg.border) == (4, 4)
    assert cfg.min_feature_distance == C.c_float(0.7).value and cfg.history == 30
    assert cfg.prune_min_kps == 30 and cfg.prune_window_ns == 1_000_000_000
    assert C.sizeof(cfg) == 32  # float, 5 x int / float, 4 bytes of padding, long long


def test_null_arguments_are_refused_without_a_device():
    from multimotionfusion_amd import _capi
    lib = _capi.load()
    cfg = _capi.mmf_keypoint_frontend_config()
    assert lib.mmf_keypoint_frontend_default_config(None) == -1
    assert b"mmf_keypoint_frontend_default_config" in lib.mmf_last_error()
    assert lib.mmf_fusion_set_keypoint_frontend(None, None, C.byref(cfg)) == -1
    assert lib.mmf_superpoint_get_features_device(None, None, 64, 48, 1, 0.015, 4, 4) == -1
    assert lib.mmf_superpoint_device_features(None, None, None, None, None, None) == -1
    assert lib.mmf_superpoint_device_status(None, None) == -1
    n = C.c_int()
    assert lib.mmf_superpoint_last_features(None, C.byref(n), None, None, None, None) == -1
    assert lib.mmf_superpoint_last_launches(None) == -1
    assert lib.mmf_tracker_add_keypoints_device(None, None, None, None, None, 0, 0.7, 30) == -1
    assert b"mmf_tracker_add_keypoints_device" in lib.mmf_last_error()
    assert lib.mmf_tracker_set_keypoint_status(None, None) == -1
    assert lib.mmf_tracker_keypoint_failures(None, C.byref(n)) == -1
