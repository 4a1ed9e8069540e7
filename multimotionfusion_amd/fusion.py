"""Host-side mirror of class MultiMotionFusion (Core/MultiMotionFusion.h:78-300): processFrame (one or many
rigid-body models), predict, getModels / getBackgroundModel / getTextures, the runtime setters, exportPoses.
The orchestration itself is native code inside libmmf_hip.so (mmf_fusion_*)."""
import ctypes as C
import weakref

import numpy as np

from . import _capi
from ._capi import check, fptr, mmf_frame, mmf_fusion_config, mmf_mask_info, mmf_segmentation, mmf_segmentation_model
from .cudafuncs import Context, _p
from .model import Model
from .odometry import RGBDOdometry

MMF_LOAD_DENSE = 1  # mmf_fusion_load_models_ex's flag
DENSE_STATUS = ("restored", "no file", "does not parse", "too large")  # MMF_DENSE_*


class HostFrame:
    """One frame in host memory (FrameData::rgb / depth as numpy arrays) with the arrays' addresses taken once: numpy's
    `.ctypes.data` costs ~2 us per access, 9 us per call for the four pointers of a frame and its successor."""
    __slots__ = ("rgb", "depth", "rgb_ptr", "depth_ptr")

    def __init__(self, rgb, depth):
        # raw addresses reach a C memcpy / DMA: the wrong dtype or stride would be an out-of-bounds host read (and an
        # `assert` disappears under python -O), so convertible inputs are converted and anything else is refused
        rgb, depth = np.ascontiguousarray(rgb), np.ascontiguousarray(depth)
        if rgb.dtype != np.uint8 or depth.dtype != np.float32:
            raise TypeError(f"HostFrame: rgb must be uint8 and depth float32 (metres), got {rgb.dtype} / {depth.dtype}")
        if rgb.ndim != 3 or rgb.shape[2] != 3 or depth.shape != rgb.shape[:2]:
            raise TypeError(f"HostFrame: rgb (H, W, 3) and depth (H, W) expected, got {rgb.shape} / {depth.shape}")
        self.rgb, self.depth = rgb, depth  # (kept alive with the addresses)
        self.rgb_ptr, self.depth_ptr = rgb.ctypes.data, depth.ctypes.data


class MultiMotionFusion:
    def __init__(self, ctx: Context, width, height, cx, cy, fx, fy, **overrides):
        self.ctx, self.width, self.height = ctx, width, height
        cfg = mmf_fusion_config()
        check(ctx.lib.mmf_fusion_default_config(C.byref(cfg)))
        for k, v in overrides.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown MultiMotionFusion option {k}")
            setattr(cfg, k, v)
        self.config = cfg
        h = C.c_void_p()
        check(ctx.lib.mmf_fusion_create(ctx.handle, width, height, cx, cy, fx, fy, C.byref(cfg), C.byref(h)))
        self.handle = h
        ctx._children.append(weakref.ref(self))
        # borrowed views of the objects the fusion owns
        self._model = self._borrow_model(ctx.lib.mmf_fusion_model(h))
        self._odom = self._borrow_odom(ctx.lib.mmf_fusion_odometry(h))
        from .segmentation import MaskConfig
        self._mask, self._mask_on = MaskConfig(), False  # (setMaskSegmentation)

    def _borrow_model(self, handle):
        m = Model.__new__(Model)
        m.ctx, m.width, m.height = self.ctx, self.width, self.height
        m.handle = C.c_void_p(handle)
        m.id = self.ctx.lib.mmf_model_id(m.handle)
        m.close = lambda: None
        return m

    def _borrow_odom(self, handle):
        o = RGBDOdometry.__new__(RGBDOdometry)
        o.ctx, o.width, o.height = self.ctx, self.width, self.height
        o.handle = C.c_void_p(handle)
        o.close = lambda: None
        return o

    def processFrame(self, rgb, depth, timestamp=0, inPose=None, weightMultiplier=1.0, bootstrap=False, initTransform=None,
                     icpRefine=True, mask=None, hasNewLabel=False, modelData=None, initTransforms=None, next=None):
        """MultiMotionFusion::processFrame: rgb [H,W,3] uint8, depth [H,W] float32 (CUDA tensors).
        initTransform: `-init kp` (MultiMotionFusion.cpp:312-384) -- the 4x4 of Model::getLastTrackTransform, applied
        to the pose before the dense tracker (which then refines it when icpRefine, `-icp_refine`).
        mask / hasNewLabel / modelData: the SegmentationResult of this frame when enable_multiple_models is set
        (fullSegmentation as a CUDA uint8 [H,W] tensor of model ids; modelData: dicts with id, super_pixel_count,
        avg_confidence, depth_mean, depth_std in list order).  With setMaskSegmentation on, a mask without modelData is the
        frame's RAW label image and hasNewLabel is ignored.  initTransforms: one 4x4 per active model.
        next: (rgb, depth) the NEXT call will be given -- prefetchFrame folded into this call: the next frame's
        sensor-side preparation is enqueued while this one waits for its pose (mmf_frame::next_rgb / next_depth)."""
        if mask is not None or initTransforms is not None or next is not None:
            fr = mmf_frame()
            fr.rgb, fr.depth, fr.timestamp = _p(rgb), _p(depth), int(timestamp)
            if next is not None:
                fr.next_rgb, fr.next_depth = _p(next[0]), _p(next[1])
            if initTransform is not None:
                assert initTransforms is None
                initTransforms = [initTransform]
            fr.weight_multiplier, fr.bootstrap, fr.icp_refine = float(weightMultiplier), int(bool(bootstrap)), int(bool(icpRefine))
            keep = []
            if inPose is not None:
                pose = np.ascontiguousarray(np.asarray(inPose, np.float32).reshape(16))
                keep.append(pose)
                fr.in_pose = fptr(pose)
            if initTransforms is not None:
                T = np.ascontiguousarray(np.asarray(initTransforms, np.float32).reshape(-1, 16))
                keep.append(T)
                fr.init_transforms, fr.n_init_transforms = fptr(T), T.shape[0]
            if mask is not None:
                seg = mmf_segmentation()
                seg.mask, seg.has_new_label = _p(mask), int(bool(hasNewLabel))
                if modelData:
                    arr = (mmf_segmentation_model * len(modelData))()
                    for i, d in enumerate(modelData):
                        arr[i].id, arr[i].super_pixel_count = int(d["id"]), int(d["super_pixel_count"])
                        arr[i].avg_confidence = float(d["avg_confidence"])
                        arr[i].depth_mean, arr[i].depth_std = float(d["depth_mean"]), float(d["depth_std"])
                    seg.n_models, seg.model_data = len(modelData), arr
                    keep.append(arr)
                keep.append(seg)
                fr.segmentation = C.pointer(seg)
            check(self.ctx.lib.mmf_fusion_process_frame_ex(self.handle, C.byref(fr)))
            return
        if initTransform is not None:
            assert inPose is None and not bootstrap
            T = np.ascontiguousarray(np.asarray(initTransform, np.float32).reshape(16))
            check(self.ctx.lib.mmf_fusion_process_frame_init(self.handle, _p(rgb), _p(depth), int(timestamp), fptr(T),
                                                             int(bool(icpRefine)), float(weightMultiplier)))
            return
        pose = None
        if inPose is not None:
            pose = np.ascontiguousarray(np.asarray(inPose, np.float32).reshape(16))
        check(self.ctx.lib.mmf_fusion_process_frame(self.handle, _p(rgb), _p(depth), int(timestamp),
                                                    fptr(pose) if pose is not None else None,
                                                    float(weightMultiplier), int(bool(bootstrap))))

    def prefetchFrame(self, rgb, depth):
        """Start the depth filter and the input-side preparation of the NEXT frame on a second stream (they overlap
        the fusion of the current one).  The next processFrame call must get the same tensors, unchanged."""
        check(self.ctx.lib.mmf_fusion_prefetch_frame(self.handle, _p(rgb), _p(depth)))

    def reset(self):
        check(self.ctx.lib.mmf_fusion_reset(self.handle))

    def getCurrPose(self):
        p = np.zeros(16, np.float32)
        check(self.ctx.lib.mmf_fusion_get_pose(self.handle, fptr(p)))
        return p.reshape(4, 4)

    def getTick(self):
        return self.ctx.lib.mmf_fusion_tick(self.handle)

    def getBackgroundModel(self):
        return self._model

    def getModels(self):
        """std::list<std::shared_ptr<Model>>& getModels(): the active models in list order (index 0 = global)."""
        lib = self.ctx.lib
        return [self._borrow_model(lib.mmf_fusion_model_at(self.handle, i)) for i in range(lib.mmf_fusion_num_models(self.handle))]

    def getInactiveModels(self):
        lib = self.ctx.lib
        return [self._borrow_model(lib.mmf_fusion_inactive_model_at(self.handle, i))
                for i in range(lib.mmf_fusion_num_inactive_models(self.handle))]

    def getModelOdometry(self, index):
        o = self._borrow_odom(self.ctx.lib.mmf_fusion_odometry_at(self.handle, index))
        o._refresh_stats()
        return o

    def getNextModelID(self):
        return self.ctx.lib.mmf_fusion_next_model_id(self.handle)

    def scheduleDeactivation(self, model_id):
        check(self.ctx.lib.mmf_fusion_schedule_deactivation(self.handle, int(model_id)))

    def processFrameHost(self, rgb, depth=None, timestamp=0, mask=None, hasNewLabel=False, inPose=None, weightMultiplier=1.0,
                         bootstrap=False, next=None):
        """processFrame(const FrameData&) with HOST numpy arrays: staged through pinned buffers and uploaded inside.
        next = (rgb, depth) of the NEXT call (C-contiguous uint8 / float32 arrays, the very objects that call will pass):
        uploaded and prepared during this one (mmf_fusion_process_frame_host_next).  A frame may also be handed in as a
        HostFrame (rgb=HostFrame, next=HostFrame): the arrays' addresses are then taken once, not per call."""
        cur = rgb if isinstance(rgb, HostFrame) else HostFrame(rgb, depth)
        nxt = None if next is None else (next if isinstance(next, HostFrame) else HostFrame(*next))
        m = np.ascontiguousarray(mask, np.uint8) if mask is not None else None
        pose = np.ascontiguousarray(np.asarray(inPose, np.float32).reshape(16)) if inPose is not None else None
        check(self.ctx.lib.mmf_fusion_process_frame_host_next(
            self.handle, cur.rgb_ptr, cur.depth_ptr, m.ctypes.data if m is not None else None, int(bool(hasNewLabel)),
            int(timestamp), fptr(pose) if pose is not None else None, float(weightMultiplier), int(bool(bootstrap)),
            nxt.rgb_ptr if nxt is not None else None, nxt.depth_ptr if nxt is not None else None))

    def predict(self):
        check(self.ctx.lib.mmf_fusion_predict(self.handle))

    def setShard(self, rank, world):
        """Per-rigid-body shard: this process runs the models whose list index k has k % world == rank."""
        check(self.ctx.lib.mmf_fusion_set_shard(self.handle, int(rank), int(world)))

    def ownsModel(self, index):
        return bool(self.ctx.lib.mmf_fusion_owns_model(self.handle, int(index)))

    def setModelPose(self, index, pose):
        p = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(16))
        check(self.ctx.lib.mmf_fusion_set_model_pose(self.handle, int(index), fptr(p)))

    def lastTimings(self):
        a, b = C.c_double(), C.c_double()
        check(self.ctx.lib.mmf_fusion_last_timings(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def setTick(self, val):
        check(self.ctx.lib.mmf_fusion_set_tick(self.handle, int(val)))

    def _set(self, name, val):
        check(getattr(self.ctx.lib, "mmf_fusion_set_" + name)(self.handle, val))

    def setRgbOnly(self, v): self._set("rgb_only", int(bool(v)))
    def setIcpWeight(self, v): self._set("icp_weight", float(v))
    def setOutlierCoefficient(self, v): self._set("outlier_coefficient", float(v))
    def setPyramid(self, v): self._set("pyramid", int(bool(v)))
    def setFastOdom(self, v): self._set("fast_odom", int(bool(v)))
    def setSo3(self, v): self._set("so3", int(bool(v)))
    def setFrameToFrameRGB(self, v): self._set("frame_to_frame_rgb", int(bool(v)))
    def setDepthCutoff(self, v): self._set("depth_cutoff", float(v))
    def setConfidenceThreshold(self, v): self._set("confidence_threshold", float(v))
    def setEnableMultipleModels(self, v): self._set("enable_multiple_models", int(bool(v)))

    # ----- the built-in dense-CRF segmentation (segmentation.py) and the settings of MultiMotionFusion.h:243-261 that feed it
    def setCrfSegmentation(self, cfg=True):
        """cfg: a segmentation.CrfConfig (True: the current settings); None / False: off (the default).  With it on and no
        mask or callback, processFrame computes the segmentation of every multi-model tracked frame itself."""
        from .segmentation import CrfConfig
        if cfg is None or cfg is False:
            self._crf_on = False
            check(self.ctx.lib.mmf_fusion_set_crf_segmentation(self.handle, None))
            return
        if cfg is not True:
            self._crf = cfg
        elif not hasattr(self, "_crf"):
            self._crf = CrfConfig()
        self._crf_on = True
        check(self.ctx.lib.mmf_fusion_set_crf_segmentation(self.handle, C.byref(self._crf.to_c())))

    def _crf_set(self, name, v):
        from .segmentation import CrfConfig
        if not hasattr(self, "_crf"):
            self._crf = CrfConfig()
        setattr(self._crf, name, v)
        # (the settings reach the fusion with the CRF off too -- the spawn-offset counter runs either way -- and it stays off)
        check(self.ctx.lib.mmf_fusion_set_crf_segmentation(self.handle, C.byref(self._crf.to_c())))
        if not getattr(self, "_crf_on", False):
            check(self.ctx.lib.mmf_fusion_set_crf_segmentation(self.handle, None))

    def setCrfPairwiseSigmaRGB(self, v): self._crf_set("sigma_rgb", float(v))
    def setCrfPairwiseSigmaPosition(self, v): self._crf_set("sigma_pos", float(v))
    def setCrfPairwiseSigmaDepth(self, v): self._crf_set("sigma_depth", float(v))
    def setCrfPairwiseWeightAppearance(self, v): self._crf_set("weight_appearance", float(v))
    def setCrfPairwiseWeightSmoothness(self, v): self._crf_set("weight_smoothness", float(v))
    def setCrfThresholdNew(self, v): self._crf_set("threshold_new", float(v))
    def setCrfUnaryWeightError(self, v): self._crf_set("unary_weight_error", float(v))
    def setCrfUnaryKError(self, v): self._crf_set("unary_k_error", float(v))
    def setCrfIteration(self, v): self._crf_set("iterations", int(v))
    def setNewModelMinRelativeSize(self, v): self._crf_set("min_rel_size_new", float(v))
    def setNewModelMaxRelativeSize(self, v): self._crf_set("max_rel_size_new", float(v))
    def setModelSpawnOffset(self, v):
        self._crf_set("model_spawn_offset", int(v))
        self._mask_set("model_spawn_offset", int(v))

    def setSetInhibit(self, v):
        self._crf_set("inhibit_new", int(bool(v)))
        self._mask_set("inhibit_new", int(bool(v)))

    # ----- the segmentation from a frame's own label image (Segmentation.cpp:89-147; segmentation.mask_segment)
    def setMaskSegmentation(self, cfg=True):
        """cfg: a segmentation.MaskConfig (True: the current settings); None / False: off (the default).  With it on, a
        mask handed to processFrame / processFrameHost WITHOUT modelData is the frame's raw label image (Mask####.png,
        ground-truth ids, an instance segmenter's output): processFrame maps it to model ids through its persistent table,
        spawns a model for the raster-first new label and computes the model data itself; hasNewLabel is ignored."""
        if cfg is None or cfg is False:
            self._mask_on = False
            check(self.ctx.lib.mmf_fusion_set_mask_segmentation(self.handle, None))
            return
        if cfg is not True:
            self._mask = cfg
        self._mask_on = True
        check(self.ctx.lib.mmf_fusion_set_mask_segmentation(self.handle, C.byref(self._mask.to_c())))

    def _mask_set(self, name, v):
        setattr(self._mask, name, v)
        if self._mask_on:  # (pushed while the mode is on; kept for when it is switched on otherwise)
            check(self.ctx.lib.mmf_fusion_set_mask_segmentation(self.handle, C.byref(self._mask.to_c())))

    def maskMapping(self):
        """the persistent input label -> model id table (numpy uint8 [256]); reset() clears it"""
        out = np.zeros(256, np.uint8)
        check(self.ctx.lib.mmf_fusion_mask_mapping(self.handle, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def lastMaskSegmentation(self):
        """what the last frame segmented from its labels computed: model data (list order, then the new label's entry),
        allow_new, has_new_label as processFrame used it, new_label (the input label that became new, or -1)"""
        from .segmentation import model_data_dicts
        info = mmf_mask_info()
        check(self.ctx.lib.mmf_fusion_last_mask_segmentation(self.handle, C.byref(info), None, 0))
        md = (mmf_segmentation_model * max(info.n_models, 1))()
        check(self.ctx.lib.mmf_fusion_last_mask_segmentation(self.handle, C.byref(info), md, info.n_models))
        return dict(model_data=model_data_dicts(md, info.n_models), allow_new=bool(info.allow_new),
                    has_new_label=bool(info.has_new_label), new_label=info.new_label)

    def setSuperpixels(self, labels):
        """the super-pixel label image (int32 [H,W] CUDA tensor) of the NEXT frame's segmentation; None: the regular grid"""
        import torch
        if labels is not None:
            assert labels.dtype == torch.int32 and labels.shape == (self.height, self.width)
            labels = labels.contiguous()
        check(self.ctx.lib.mmf_fusion_set_superpixels(self.handle, _p(labels) if labels is not None else None))

    def setSuperpixelEngine(self, on):
        """the built-in segmentation computes every frame's super-pixels from its RGB on the device (SLIC);
        labels handed in through setSuperpixels still win for their frame; off (default): the regular grid"""
        check(self.ctx.lib.mmf_fusion_set_superpixel_engine(self.handle, 1 if on else 0))

    def getLastSuperpixels(self):
        """the label image (int32 [H,W] CUDA tensor) the last segmentation used: handed in, the engine's, or the grid"""
        import torch
        out = torch.empty((self.height, self.width), dtype=torch.int32, device=torch.device("cuda", self.ctx.device))
        check(self.ctx.lib.mmf_fusion_last_superpixels(self.handle, _p(out)))
        return out

    def setOpticalFlow(self, config=True):
        """every frame's dense optical flow from the frame before it, computed from its RGB on a stream of its own beside
        the tracking (flow.FarnebackFlow's engine).  True: the reference's settings; a flow.FlowConfig: those;
        False / None (the default state): off, the engine is freed.  Poses, maps and masks do not depend on it."""
        from .flow import FlowConfig
        if config is None or config is False:
            check(self.ctx.lib.mmf_fusion_set_optical_flow(self.handle, None))
            return
        cfg = FlowConfig() if config is True else config
        check(self.ctx.lib.mmf_fusion_set_optical_flow(self.handle, C.byref(cfg.c)))

    def getLastFlow(self):
        """(flow [h,w,2], magnitude [h,w], motion [h,w]) float32 CUDA tensors (copies) of the last frame, or None after the
        first frame of a sequence (creation, reset)"""
        from .flow import _result_tensors

        def getter(*a):
            has = C.c_int()
            check(self.ctx.lib.mmf_fusion_last_flow(*a, C.byref(has)))
            return bool(has.value)
        return _result_tensors(self.ctx, getter, self.handle)

    def setFlowInference(self, config=True):
        """the flow-CRF inference (flowcrf.FlowCrf's engine) on every tracked frame that has a flow, on the
        flow's stream behind it; needs setOpticalFlow.  True: the reference's settings; a flowcrf.FlowCrfConfig: those;
        False / None (the default state): off, the engine is freed.  Poses, maps and masks do not depend on it."""
        from .flowcrf import FlowCrfConfig
        if config is None or config is False:
            check(self.ctx.lib.mmf_fusion_set_flow_inference(self.handle, None))
            return
        cfg = FlowCrfConfig() if config is True else config
        check(self.ctx.lib.mmf_fusion_set_flow_inference(self.handle, C.byref(cfg.c)))

    def getLastFlowInference(self):
        """(ids [h/4,w/4], ids_full [h,w]) uint8 CUDA tensors (copies) of the last frame, or None after the first frame of a
        sequence and after a frame that was not tracked"""
        import torch
        from .model import _as_tensor
        p_ids, p_full = C.c_void_p(), C.c_void_p()
        w, h, L, has = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self.ctx.lib.mmf_fusion_last_flow_inference(self.handle, C.byref(p_ids), C.byref(p_full), C.byref(w), C.byref(h),
                                                          C.byref(L), C.byref(has)))
        if not has.value:
            return None
        self.ctx.synchronize()  # (the copies below run on torch's stream, which need not be the context's)
        ids = _as_tensor(p_ids.value, w.value * h.value, torch.uint8, (h.value, w.value), self.ctx.device, None).clone()
        full = _as_tensor(p_full.value, 16 * w.value * h.value, torch.uint8, (4 * h.value, 4 * w.value), self.ctx.device, None).clone()
        return ids, full

    def downloadFlowInference(self, name):
        """a stage image of the last frame's inference as a numpy array (tests), as flowcrf.FlowCrf.download: E / U / proj /
        Q / prob float32 [L,h/4,w/4]; label int32, ids / invalid uint8 [h/4,w/4]; ids_full uint8 [h,w]"""
        w, h, L, has = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self.ctx.lib.mmf_fusion_last_flow_inference(self.handle, None, None, C.byref(w), C.byref(h), C.byref(L), C.byref(has)))
        if name in ("E", "U", "proj", "Q", "prob"):
            out = np.empty((L.value, h.value, w.value), np.float32)
        elif name == "ids_full":
            out = np.empty((4 * h.value, 4 * w.value), np.uint8)
        else:
            out = np.empty((h.value, w.value), np.int32 if name == "label" else np.uint8)
        check(self.ctx.lib.mmf_fusion_flow_inference_download(self.handle, name.encode(), C.c_void_p(out.ctypes.data), out.nbytes))
        return out

    def setFlowSegmentation(self, config=True):
        """the reference's -segm_mode flow_crf: a frame that brings no segmentation of its own is segmented
        from the flow inference's id image -- the largest blob per model, filled, scaled up, with the model data and the new
        label's 5 % rule (flowseg.FlowSegmentation's engine); needs setFlowInference.  True: the reference's settings; a
        flowseg.FlowSegConfig: those; False / None (the default state): off, the engine is freed."""
        from .flowseg import FlowSegConfig
        if config is None or config is False:
            check(self.ctx.lib.mmf_fusion_set_flow_segmentation(self.handle, None))
            return
        cfg = FlowSegConfig() if config is True else config
        check(self.ctx.lib.mmf_fusion_set_flow_segmentation(self.handle, C.byref(cfg.c)))

    def getLastFlowSegmentation(self):
        """what the flow_crf mode computed for the last frame it handled, as flowseg.FlowSegmentation.summary(): model data,
        allow_new, has_new_label as processFrame used it, new_cells, area2 and first_cell per table entry; has_result False
        for a frame without an inference result (zero mask, no entries)"""
        from .flowseg import summary_dict
        s, has = _capi.mmf_flowseg_summary(), C.c_int()
        check(self.ctx.lib.mmf_fusion_last_flow_segmentation(self.handle, C.byref(s), C.byref(has)))
        out = summary_dict(s)
        out["has_result"] = bool(has.value)
        return out

    def setFernDatabase(self, config=True, table=None):
        """the fern keyframe database (ferns.FernDatabase's engine): behind every frame's final predict() the
        camera model's fill-in images are encoded, searched for the closest keyframe that is old enough, and added when they
        differ enough from every keyframe -- on a stream of its own.  True: the reference's settings; a ferns.FernsConfig:
        those; table: int32 [num, 6] ferns (None: ferns.make_table with seed 0); False / None (the default state): off, the
        engine is freed.  Observational: poses, maps and masks do not depend on it."""
        from .ferns import FernsConfig, _table_arg
        if config is None or config is False:
            check(self.ctx.lib.mmf_fusion_set_fern_database(self.handle, None, None))
            self._ferns_cfg = None
            return
        cfg = FernsConfig() if config is True else config
        tab = None if table is None else _table_arg(table, cfg.num)
        check(self.ctx.lib.mmf_fusion_set_fern_database(self.handle, C.byref(cfg.c), None if tab is None else tab.ctypes.data_as(C.POINTER(C.c_int))))
        self._ferns_cfg = cfg

    def getLastFernResult(self):
        """the database's record of the last frame as a dict (ferns.result_dict): added, dropped_total, count, good_codes,
        add_minimum, closest, closest_dissim, closest_similarity, candidate, closest_pose, closest_time"""
        from .ferns import result_dict
        r = _capi.mmf_ferns_result_t()
        check(self.ctx.lib.mmf_fusion_last_fern_result(self.handle, C.byref(r)))
        return result_dict(r)

    def getFernDatabase(self):
        """the hook's engine, to read from (keyframe, download, result, last_launches); None while the hook is off.  The
        handle belongs to the fusion: it is valid until the next setFernDatabase call."""
        from .ferns import _Engine
        h = self.ctx.lib.mmf_fusion_fern_database(self.handle)
        cfg = getattr(self, "_ferns_cfg", None)
        if not h or cfg is None:
            return None
        return _Engine(self.ctx, C.c_void_p(h), self.width, self.height, cfg.num, cfg.capacity)

    def getLastSegmentation(self):
        """segmentation.last() of this fusion: unaries, Q, raw and filtered maps, model data, range, B4 flag"""
        import torch
        from .segmentation import _last
        return _last(self.ctx.lib.mmf_fusion_last_segmentation, self.handle, torch.device("cuda", self.ctx.device))

    # ----- keypoint redetection of inactive models (MultiMotionFusion.cpp:489-559; redetection.py)
    def setEnableRedetection(self, on):
        """off by default; with it on, processFrame re-activates an inactive model whose stored keypoint views match the
        keypoints (setKeypoints) of a segment of the frame"""
        check(self.ctx.lib.mmf_fusion_set_redetection(self.handle, 1 if on else 0))

    def setRedetectionVerifier(self, mode):
        """where the redetection candidates are verified: 0 = host (the default), 1 = device (a fresh RigidRANSAC per view,
        all segments and inactive models of a frame in two launches)"""
        check(self.ctx.lib.mmf_fusion_set_redetection_verifier(self.handle, int(mode)))

    def redetectionHostVerified(self):
        """segments with more keypoints than the device verifier takes, verified on the host under its rule, so far"""
        return self.ctx.lib.mmf_fusion_redetection_host_verified(self.handle)

    def setKeypoints(self, xy, coordinate, descriptor):
        """the last keypoint of every currently visible track, for the NEXT processFrame only: xy [n,2] integer pixels,
        coordinate [n,3] camera frame (non-finite allowed), descriptor [n,256]"""
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        n = xy.shape[0]
        co = np.ascontiguousarray(coordinate, np.float32).reshape(n, 3)
        de = np.ascontiguousarray(descriptor, np.float32).reshape(n, 256)
        check(self.ctx.lib.mmf_fusion_set_keypoints(self.handle, n, xy.ctypes.data, co.ctypes.data, de.ctypes.data))

    def getViewStore(self):
        from .redetection import ViewStore
        h = self.ctx.lib.mmf_fusion_viewstore(self.handle)
        if not h:
            check(-1)
        return ViewStore(self.ctx, C.c_void_p(h), owner=self)

    def storeViews(self, model_id, views):
        """Model::store of an inactive model's keypoint views (redetection.ViewStore.store)"""
        return self.getViewStore().store(model_id, views)

    def getLastStoredViews(self):
        """what the last processFrame stored on deactivation (a tracker with a view log attached, redetection on):
        [dict(model_id, n_views, rows)]"""
        n = C.c_int()
        check(self.ctx.lib.mmf_fusion_last_stored_views(self.handle, None, None, None, 0, C.byref(n)))
        ids, nv, rows = (np.zeros(max(n.value, 1), np.int32) for _ in range(3))
        check(self.ctx.lib.mmf_fusion_last_stored_views(self.handle, ids.ctypes.data, nv.ctypes.data, rows.ctypes.data, n.value, C.byref(n)))
        return [dict(model_id=int(ids[k]), n_views=int(nv[k]), rows=int(rows[k])) for k in range(n.value)]

    def getLastRedetections(self):
        from .redetection import last_redetections
        return last_redetections(self.ctx, self.handle)

    # ----- keypoint tracks on the device (tracker.py): `-init kp` for every model, the models' track sets
    def setTracker(self, tracker, odom_init_kp=True, icp_refine=True):
        """attach a tracker.DevicePointTracker (None: detach; the default).  The caller adds and prunes a frame's keypoints
        before processFrame; processFrame then initialises every active model from its own tracks (odom_init_kp; the dense
        tracker refines when icp_refine), associates the tracks with the models by the frame's id image and, with
        redetection on and no setKeypoints for the frame, takes the tracker's visible keypoints.  Every call, also one
        that only changes a flag, switches the in-frame keypoint front end off: call setKeypointFrontEnd again after it."""
        check(self.ctx.lib.mmf_fusion_set_tracker(self.handle, tracker.handle if tracker is not None else None,
                                                  int(bool(odom_init_kp)), int(bool(icp_refine))))
        self._tracker = tracker  # (the fusion does not own it: kept alive here)
        self._kp_predictor = None  # (mmf_fusion_set_tracker has switched the front end off)

    def setKeypointFrontEnd(self, kp_predictor, conf_thresh=None, nms_dist=None, border=None, min_feature_distance=0.7, history=30,
                            prune_min_kps=30, prune_window_ns=int(1e9)):
        """run the keypoint half of processFrame (MultiMotionFusion.cpp:223-248) inside every processFrame call, on the
        frame's own device buffers and without a wait: superpoint.SuperPoint features -> the attached tracker's add ->
        prune.  kp_predictor = None: off (the default).  Thresholds default to the predictor's.  Needs setTracker first,
        and a later setTracker call switches it off again."""
        from ._capi import mmf_keypoint_frontend_config
        if kp_predictor is None:
            check(self.ctx.lib.mmf_fusion_set_keypoint_frontend(self.handle, None, None))
            self._kp_predictor = None
            return
        cfg = mmf_keypoint_frontend_config()
        check(self.ctx.lib.mmf_keypoint_frontend_default_config(C.byref(cfg)))
        cfg.conf_thresh = float(kp_predictor.conf_thresh if conf_thresh is None else conf_thresh)
        cfg.nms_dist = int(kp_predictor.nms_dist if nms_dist is None else nms_dist)
        cfg.border = int(kp_predictor.border if border is None else border)
        cfg.min_feature_distance, cfg.history = float(min_feature_distance), int(history)
        cfg.prune_min_kps, cfg.prune_window_ns = int(prune_min_kps), int(prune_window_ns)
        check(self.ctx.lib.mmf_fusion_set_keypoint_frontend(self.handle, kp_predictor.handle, C.byref(cfg)))
        self._kp_predictor = kp_predictor  # (not owned: kept alive here)

    def getLastTrackTransforms(self):
        """the transformations the last frame's models were initialised with, [n,4,4] in list order (n = 0: none)"""
        n = C.c_int()
        check(self.ctx.lib.mmf_fusion_last_track_transforms(self.handle, None, 0, C.byref(n)))
        T = np.zeros((max(n.value, 1), 4, 4), np.float32)
        check(self.ctx.lib.mmf_fusion_last_track_transforms(self.handle, T.ctypes.data, n.value, C.byref(n)))
        return T[:n.value]

    def setTrackBackdating(self, history):
        """back-date a spawned model's poses from its keypoint tracks (Model::refineTrackSubset; the reference passes
        history 2).  0 switches it off (the default).  Needs an attached tracker with a view log to do anything; with
        redetection on, the views the model stores on deactivation then reach back before its spawn."""
        check(self.ctx.lib.mmf_fusion_set_track_backdating(self.handle, int(history)))

    def getLastBackdatedPoses(self):
        """(model id, [entry dicts, oldest first]) of what the last processFrame back-dated; (-1, []) when nothing"""
        from ._capi import mmf_backdated_pose
        from .tracker import backdated_pose_dict
        n, mid = C.c_int(), C.c_int()
        check(self.ctx.lib.mmf_fusion_last_backdated_poses(self.handle, C.byref(mid), None, 0, C.byref(n)))
        out = (mmf_backdated_pose * max(n.value, 1))()
        check(self.ctx.lib.mmf_fusion_last_backdated_poses(self.handle, C.byref(mid), out, n.value, C.byref(n)))
        return mid.value, [backdated_pose_dict(out[j]) for j in range(n.value)]

    def getConfig(self):
        cfg = mmf_fusion_config()
        check(self.ctx.lib.mmf_fusion_get_config(self.handle, C.byref(cfg)))
        return cfg

    def getTexture(self, name):
        """getTextures()[name]: "RGB", "DEPTH_METRIC", "DEPTH_METRIC_FILTERED", "MASK" as a CUDA tensor view."""
        import torch
        from .model import _as_tensor
        p, b = C.c_void_p(), C.c_size_t()
        check(self.ctx.lib.mmf_fusion_texture(self.handle, name.encode(), C.byref(p), C.byref(b)))
        dt = torch.uint8 if name in ("RGB", "MASK") else torch.float32
        shape = (self.height, self.width, 3) if name == "RGB" else (self.height, self.width)
        return _as_tensor(p.value, b.value, dt, shape, self.ctx.device, self)

    def getErrorTexture(self, index, which="icp"):
        """Model::getICPErrorTexture / getRGBErrorTexture of the index-th active model (CUDA float32 [H,W] view)."""
        import torch
        from .model import _as_tensor
        p = C.c_void_p()
        check(self.ctx.lib.mmf_fusion_error_texture(self.handle, int(index), 0 if which == "icp" else 1, C.byref(p)))
        return _as_tensor(p.value, self.width * self.height * 4, torch.float32, (self.height, self.width), self.ctx.device, self)

    def exportPoses(self, export_dir):
        check(self.ctx.lib.mmf_fusion_export_poses(self.handle, export_dir.encode()))

    def savePly(self, exportDir):
        """MultiMotionFusion::savePly (:1001-1018): cloud-<id>.ply per model under exportDir and the model database
        (model_db/model-<id>/cloud.ply, tracks.ply for models with stored views); modeldb.py reads the files"""
        check(self.ctx.lib.mmf_fusion_save_models(self.handle, str(exportDir).encode()))

    def loadModels(self, exportDir, dense=False):
        """MultiMotionFusion::loadModels (:131-145, -restore): every model_db/model-<id>/tracks.ply under exportDir becomes
        an inactive object model with the next id and the file's views -> the number of models loaded.  dense=True (ours, the
        reference restores no surfels): the records of model_db/model-<id>/cloud.ply become the model's surfels, stable, with
        the tick of the load as both times; the frame that activates the model moves their timestamps into its window."""
        n = C.c_int()
        if dense:
            check(self.ctx.lib.mmf_fusion_load_models_ex(self.handle, str(exportDir).encode(), MMF_LOAD_DENSE, C.byref(n)))
        else:
            check(self.ctx.lib.mmf_fusion_load_models(self.handle, str(exportDir).encode(), C.byref(n)))
        return n.value

    def getLastDenseRestores(self):
        """per model of the last loadModels(dense=True): dict(model_id, surfels, status), status one of DENSE_STATUS"""
        from ._capi import mmf_dense_restore
        n = C.c_int()
        check(self.ctx.lib.mmf_fusion_last_dense_restores(self.handle, None, 0, C.byref(n)))
        arr = (mmf_dense_restore * max(n.value, 1))()
        check(self.ctx.lib.mmf_fusion_last_dense_restores(self.handle, arr, n.value, C.byref(n)))
        return [dict(model_id=r.model_id, surfels=r.surfels, status=DENSE_STATUS[r.status]) for r in arr[:n.value]]

    def getPoseLog(self, index=0):
        n = C.c_int()
        check(self.ctx.lib.mmf_fusion_pose_log(self.handle, index, None, None, 0, C.byref(n)))
        ts = np.zeros(n.value, np.int64)
        p7 = np.zeros((n.value, 7), np.float32)
        if n.value:
            check(self.ctx.lib.mmf_fusion_pose_log(self.handle, index, ts.ctypes.data_as(C.POINTER(C.c_longlong)), fptr(p7),
                                                   n.value, C.byref(n)))
        return ts, p7

    def getFrameOdometry(self):
        self._odom._refresh_stats()
        return self._odom

    def close(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.mmf_fusion_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
