"""SuperPoint keypoints on the device: the host-side mirror of the `SuperPoint` class the reference takes from
the super_point_inference package (Core/MultiMotionFusion.h:46,366; MultiMotionFusion.cpp:78,233), over the C
ABI -- no fallback.

    kp = SuperPoint(ctx, weights, max_width=640, max_height=480)
    coordinates, descriptors = kp.getFeatures(img)        # [n,2] float64 in [0,1), [n,256] float64

`precision="f16"` runs the forward pass with f16 operands and f32 accumulation; the default is "f32".
"""
import ctypes as C
import weakref

import numpy as np
import torch

from .cudafuncs import Context, _p, check

LAYERS = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convPb", "convDa",
          "convDb")


SHAPES = ((1, 64, 3), (64, 64, 3), (64, 64, 3), (64, 64, 3), (64, 128, 3), (128, 128, 3), (128, 128, 3), (128, 128, 3),
          (128, 256, 3), (256, 65, 1), (128, 256, 3), (256, 256, 1))  # (Cin, Cout, k) of LAYERS


def random_weights(seed=0):
    """He-initialised weights of the SuperPointNet architecture (there is no network access for the MagicLeap
    checkpoint): what bench.py and tools/ run the network on."""
    rng = np.random.default_rng(seed)
    return [(rng.normal(0, np.sqrt(2.0 / (ci * k * k)), (co, ci, k, k)).astype(np.float32),
             rng.normal(0, 0.05, co).astype(np.float32)) for ci, co, k in SHAPES]


def forward_flops(width, height):
    """multiply-adds * 2 of one forward pass (convolutions only)"""
    total, h, w = 0, height, width
    for i, (ci, co, k) in enumerate(SHAPES):
        if i in (2, 4, 6):
            h, w = h // 2, w // 2
        total += 2 * h * w * ci * co * k * k
    return total


def load_weights(path):
    """The 12 (weight, bias) pairs of a SuperPointNet checkpoint: a TorchScript archive (what the reference's
    `-model SuperPointNet.pt` points at) or a plain state dict.  File plumbing only."""
    try:
        sd = torch.jit.load(path, map_location="cpu").state_dict()
    except Exception:
        sd = torch.load(path, map_location="cpu")
        if hasattr(sd, "state_dict"):
            sd = sd.state_dict()
    return [(sd[f"{n}.weight"].float().numpy(), sd[f"{n}.bias"].float().numpy()) for n in LAYERS]


PRECISIONS = {"f32": 0, "f16": 1}  # MMF_SP_F32, MMF_SP_F16

# (cout, shift of the output's sides) of forwardPrefix(img, layers), layers = 1..9
PREFIX_SHAPES = ((64, 0), (64, 1), (64, 1), (64, 2), (128, 2), (128, 3), (128, 3), (128, 3), (512, 3))


def f16_round(a):
    """the library's f32 -> f16 rounding (mmf_f16_round): the bits as a uint16 array of a's shape"""
    from . import _capi
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty(a.shape, np.uint16)
    check(_capi.load().mmf_f16_round(a.ctypes.data, a.size, out.ctypes.data))
    return out


class SuperPoint:
    def __init__(self, ctx: Context, weights, max_width=640, max_height=480, max_keypoints=4096, conf_thresh=0.015,
                 nms_dist=4, border=4, precision="f32"):
        if isinstance(weights, str):
            weights = load_weights(weights)
        assert len(weights) == 12
        flat = []
        for w, b in weights:
            flat += [np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)]
        arr = (C.c_void_p * 24)(*[a.ctypes.data for a in flat])
        self.ctx, self.lib = ctx, ctx.lib
        self.max_keypoints = int(max_keypoints)
        self.conf_thresh, self.nms_dist, self.border = float(conf_thresh), int(nms_dist), int(border)
        h = C.c_void_p()
        code = PRECISIONS.get(precision, precision)  # (an unknown value goes to the library, which refuses it)
        if precision == "f32":
            check(self.lib.mmf_superpoint_create(ctx.handle, arr, int(max_width), int(max_height), self.max_keypoints, C.byref(h)))
        else:
            check(self.lib.mmf_superpoint_create_ex(ctx.handle, arr, int(max_width), int(max_height), self.max_keypoints, int(code),
                                                    C.byref(h)))
        self.handle = h
        self._size = None
        ctx._children.append(weakref.ref(self))

    def _image(self, img):
        if not isinstance(img, torch.Tensor):
            img = torch.from_numpy(np.ascontiguousarray(img, np.uint8)).cuda(self.ctx.device)
        assert img.dtype == torch.uint8 and img.is_cuda and img.dim() in (2, 3)
        img = img.contiguous()
        return img, img.shape[0], img.shape[1], 1 if img.dim() == 2 else img.shape[2]

    def forward(self, img):
        """Runs the network; returns (semi [H/8,W/8,65], desc [H/8,W/8,256], heat [H,W]) as numpy arrays."""
        img, H, W, ch = self._image(img)
        check(self.lib.mmf_superpoint_forward(self.handle, _p(img), W, H, ch))
        out = []
        for which, shape in enumerate(((H // 8, W // 8, 65), (H // 8, W // 8, 256), (H, W))):
            a = np.empty(shape, np.float32)
            check(self.lib.mmf_superpoint_download(self.handle, which, a.ctypes.data, a.size))
            out.append(a)
        return tuple(out)

    @property
    def precision(self):
        return {v: k for k, v in PRECISIONS.items()}[self.lib.mmf_superpoint_precision(self.handle)]

    def forwardPrefix(self, img, layers):
        """(tests, tools) the first `layers` launches of the forward pass (1 = conv1a ... 9 = the fused 3x3 head) and that
        launch's output [h,w,cout]: float16 on an f16 object, float32 on an f32 one"""
        img, H, W, ch = self._image(img)
        cout, shift = PREFIX_SHAPES[int(layers) - 1]
        a = np.empty((H >> shift, W >> shift, cout), np.float16 if self.precision == "f16" else np.float32)
        check(self.lib.mmf_debug_superpoint_forward_prefix(self.handle, _p(img), W, H, ch, int(layers), a.ctypes.data, a.nbytes))
        return a

    def enqueue(self, img):
        """forward pass only, asynchronous (bench)"""
        img, H, W, ch = self._image(img)
        check(self.lib.mmf_superpoint_forward(self.handle, _p(img), W, H, ch))

    def keypoints(self, img):
        """(xy [n,2] int32 pixels, conf [n] float32, desc [n,256] float32), strongest first"""
        img, H, W, ch = self._image(img)
        xy = np.empty((self.max_keypoints, 2), np.int32)
        conf = np.empty(self.max_keypoints, np.float32)
        desc = np.empty((self.max_keypoints, 256), np.float32)
        n = C.c_int(0)
        check(self.lib.mmf_superpoint_get_features(self.handle, _p(img), W, H, ch, self.conf_thresh, self.nms_dist, self.border,
                                                   xy.ctypes.data, conf.ctypes.data, desc.ctypes.data, C.byref(n)))
        return xy[:n.value].copy(), conf[:n.value].copy(), desc[:n.value].copy()

    def getFeaturesDevice(self, img):
        """keypoints(img) without the host: enqueued on the context's stream, nothing awaited or read back.  The results stay
        on the device (deviceFeatures); lastFeatures() fetches them."""
        img, H, W, ch = self._image(img)
        check(self.lib.mmf_superpoint_get_features_device(self.handle, _p(img), W, H, ch, self.conf_thresh, self.nms_dist, self.border))

    def deviceFeatures(self):
        """DEVICE addresses of the last getFeaturesDevice's results, owned by this object: (count, status, xy, conf, desc)"""
        cnt, status, xy, conf, desc = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(self.lib.mmf_superpoint_device_features(self.handle, C.byref(cnt), C.byref(xy), C.byref(conf), C.byref(desc), None))
        check(self.lib.mmf_superpoint_device_status(self.handle, C.byref(status)))
        return cnt.value, status.value, xy.value, conf.value, desc.value

    def lastFeatures(self):
        """waits: (xy [n,2] int32, conf [n] float32, desc [n,256] float32, status) of the last getFeaturesDevice; status 0 =
        the suppression converged, 1 = it did not (then n = 0)"""
        xy = np.empty((self.max_keypoints, 2), np.int32)
        conf = np.empty(self.max_keypoints, np.float32)
        desc = np.empty((self.max_keypoints, 256), np.float32)
        n, status = C.c_int(0), C.c_int(0)
        check(self.lib.mmf_superpoint_last_features(self.handle, C.byref(n), C.byref(status), xy.ctypes.data, conf.ctypes.data,
                                                    desc.ctypes.data))
        return xy[:n.value].copy(), conf[:n.value].copy(), desc[:n.value].copy(), status.value

    def lastLaunches(self):
        """kernel launches of the last getFeaturesDevice (of the last selectDevice: the selection's alone)"""
        return self.lib.mmf_superpoint_last_launches(self.handle)

    def _map(self, a, shape):
        if a is None:
            return None
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.array(a, np.float32, order="C")).cuda(self.ctx.device)  # (a copy: a may be read-only)
        assert a.dtype == torch.float32 and a.is_cuda and tuple(a.shape) == shape, (tuple(a.shape), shape)
        return a.contiguous()

    def setMaps(self, width, height, semi=None, heat=None, desc=None, normalize_desc=False):
        """(tests, tools) installs maps as if a forward pass of width x height had produced them: exactly one of semi
        [H/8,W/8,65] and heat [H,W]; desc [H/8,W/8,256] or None (zeros), normalised per cell on request"""
        W, H = int(width), int(height)
        semi, heat = self._map(semi, (H // 8, W // 8, 65)), self._map(heat, (H, W))
        desc = self._map(desc, (H // 8, W // 8, 256))
        check(self.lib.mmf_superpoint_set_maps(self.handle, W, H, _p(semi) if semi is not None else None,
                                               _p(heat) if heat is not None else None, _p(desc) if desc is not None else None,
                                               int(bool(normalize_desc))))
        self.ctx.synchronize()  # the sources may go now

    def download(self, which, width, height):
        """0 logits, 1 coarse descriptors, 2 heat map of the installed maps or the last forward pass"""
        H, W = int(height), int(width)
        a = np.empty(((H // 8, W // 8, 65), (H // 8, W // 8, 256), (H, W))[which], np.float32)
        check(self.lib.mmf_superpoint_download(self.handle, which, a.ctypes.data, a.size))
        return a

    def select(self, conf_thresh=None, nms_dist=None, border=None):
        """keypoints() without the network, on the installed maps"""
        xy = np.empty((self.max_keypoints, 2), np.int32)
        conf = np.empty(self.max_keypoints, np.float32)
        desc = np.empty((self.max_keypoints, 256), np.float32)
        n = C.c_int(0)
        check(self.lib.mmf_superpoint_select(self.handle, self.conf_thresh if conf_thresh is None else float(conf_thresh),
                                             self.nms_dist if nms_dist is None else int(nms_dist),
                                             self.border if border is None else int(border), xy.ctypes.data, conf.ctypes.data,
                                             desc.ctypes.data, C.byref(n)))
        return xy[:n.value].copy(), conf[:n.value].copy(), desc[:n.value].copy()

    def selectDevice(self, conf_thresh=None, nms_dist=None, border=None):
        """getFeaturesDevice() without the network, on the installed maps; lastFeatures() fetches the results"""
        check(self.lib.mmf_superpoint_select_device(self.handle, self.conf_thresh if conf_thresh is None else float(conf_thresh),
                                                    self.nms_dist if nms_dist is None else int(nms_dist),
                                                    self.border if border is None else int(border)))

    def getFeatures(self, img):
        """SuperPoint::getFeatures as MultiMotionFusion.cpp:233 consumes it: (coordinates [n,2] float64 normalised
        by (width, height), descriptors [n,256] float64)."""
        img, H, W, _ = self._image(img)
        xy, _, desc = self.keypoints(img)
        return xy.astype(np.float64) / np.array([W, H], np.float64), desc.astype(np.float64)

    def close(self):
        if self.handle:
            self.lib.mmf_superpoint_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def conv(ctx: Context, x: torch.Tensor, w, b, relu=True, pool=False, nt=0):
    """One layer by itself: x [H,W,Cin] float32 CUDA tensor (channels last), w [Cout,Cin,k,k], b [Cout] numpy."""
    assert x.dtype == torch.float32 and x.is_cuda and x.dim() == 3
    x = x.contiguous()
    w, b = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
    H, W, cin = x.shape
    cout, taps = w.shape[0], w.shape[2] * w.shape[3]
    out = torch.empty((H // 2, W // 2, cout) if pool else (H, W, cout), dtype=torch.float32, device=x.device)
    check(ctx.lib.mmf_superpoint_conv(ctx.handle, _p(x), H, W, cin, w.ctypes.data, b.ctypes.data, cout, taps, int(relu),
                                      int(pool), int(nt), _p(out)))
    return out


def conv_f16(ctx: Context, x: torch.Tensor, w, b, relu=True, pool=False, nt=0, out_f32=False):
    """One layer of the f16 path by itself: x [H,W,Cin] float16 CUDA tensor (channels last), w [Cout,Cin,k,k], b [Cout] float32
    numpy (w is rounded to f16 as an f16 SuperPoint rounds it).  Returns float16, or the unrounded float32 with out_f32."""
    assert x.dtype == torch.float16 and x.is_cuda and x.dim() == 3
    x = x.contiguous()
    w, b = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
    H, W, cin = x.shape
    cout, taps = w.shape[0], w.shape[2] * w.shape[3]
    out = torch.empty((H // 2, W // 2, cout) if pool else (H, W, cout), dtype=torch.float32 if out_f32 else torch.float16,
                      device=x.device)
    check(ctx.lib.mmf_superpoint_conv_f16(ctx.handle, _p(x), H, W, cin, w.ctypes.data, b.ctypes.data, cout, taps, int(relu),
                                          int(pool), int(nt), int(bool(out_f32)), _p(out)))
    return out
