"""Python front end over the C-ABI (used by tests and bench.py).

Device memory is handed over as torch CUDA tensors (PyTorch is plumbing here: allocation, streams,
torch.distributed); every computation runs in libopk_hip.so.  The function names mirror the
reference operators they replace (include/opk.h lists the reference file:line of each).
"""
import atexit
import ctypes
import os
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import OpkError, check, int4
from .pose_tables import (BODY_25, CONNECT_CPU, CONNECT_GPU, CONNECT_INTER_MIN_ABOVE_THRESHOLD,
                          CONNECT_INTER_THRESHOLD,
                          CONNECT_MIN_SUBSET_CNT, CONNECT_MIN_SUBSET_SCORE, NMS_THRESHOLD)

# heat-map semantics (include/opk.h OPK_MAPS_*): the reference's CPU build or its CUDA build
MAPS_CPU, MAPS_CUDA = 0, 1
PRECISION_FP16, PRECISION_SPLIT = 0, 1      # opk_net_set_precision
CAST_CPU, CAST_CUDA = 0, 1                  # OpOutputToCvMat's branch (OPK_CAST_*)
LAYER_POSE, LAYER_FACE, LAYER_HAND = 0, 1, 2   # opk_render_layer.kind (OPK_LAYER_*)
# the renderers' default render threshold of each layer kind (alpha 0.6 for all)
_LAYER_THRESHOLD = {LAYER_POSE: 0.05, LAYER_FACE: 0.4, LAYER_HAND: 0.2}


class RenderLayer:
    """One keypoint layer of Context.render_frames: keypoints float32 CUDA [sum(counts), parts, 3]
    in output pixels, frame 0's people first (None when there are none); counts: people (faces,
    hands) of each frame."""

    def __init__(self, kind, keypoints, counts, threshold=None, alpha=0.6, pose_model=BODY_25,
                 googly_eyes=False):
        self.kind, self.keypoints, self.counts = kind, keypoints, list(counts)
        self.threshold = _LAYER_THRESHOLD[kind] if threshold is None else threshold
        self.alpha, self.pose_model, self.googly_eyes = alpha, pose_model, googly_eyes


# opk_render_heat.kind (OPK_HEAT_*); HEAT_NONE is render_element's answer for the keypoints
HEAT_NONE, HEAT_PART, HEAT_PARTS, HEAT_PAF, HEAT_PAFS, HEAT_DISTANCE = 0, 1, 2, 3, 4, 5


class RenderHeat:
    """The heat layer of Context.render_frames: what render_heat_map (HEAT_PART; HEAT_DISTANCE),
    render_heat_maps (HEAT_PARTS) or render_pafs (HEAT_PAF: channel = its x channel; HEAT_PAFS)
    draws on each frame from heat float32 CUDA [n, channels, hh, hw], frame pixel x sampling
    (x + 0.5) / scale - 0.5."""

    def __init__(self, kind, heat, scale, channel=0, alpha=0.7, pose_model=BODY_25):
        self.kind, self.heat, self.scale, self.channel = kind, heat, scale, channel
        self.alpha, self.pose_model = alpha, pose_model


def render_element(pose_model, element):
    """(HEAT_* kind, channel) of op::PoseGpuRenderer::renderPose's element (--part_to_show)."""
    kind, channel = ctypes.c_int(0), ctypes.c_int(0)
    check(_lib.load().opk_render_element(pose_model, element, ctypes.byref(kind),
                                         ctypes.byref(channel)))
    return kind.value, channel.value


def _row_bytes(t, n, h, w):
    """dst_step of a uint8 image batch: [n, h, w, 3], or [n, h, row bytes] with padded rows."""
    assert t.dtype == torch.uint8 and t.is_contiguous() and t.shape[0] == n and t.shape[1] == h
    step = t.shape[2] * 3 if t.dim() == 4 else t.shape[2]
    assert (t.dim() == 3 or t.shape[3] == 3) and step >= w * 3
    return step


def _frame_rows(t, width=None):
    """(n, h, w, row bytes) of a uint8 frame batch: [n, h, w, 3], or [n, h, row bytes] with padded
    rows of `width` pixels (the source side of _row_bytes)."""
    assert t.dtype == torch.uint8 and t.dim() in (3, 4)
    if t.dim() == 4:
        assert t.shape[3] == 3 and width in (None, t.shape[2])
        return t.shape[0], t.shape[1], t.shape[2], t.shape[2] * 3
    assert width is not None and t.shape[2] >= width * 3, "padded rows need the frame width"
    return t.shape[0], t.shape[1], width, t.shape[2]


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA tensors"
    return ctypes.c_void_p(t.data_ptr())


FRAMES_BGR, FRAMES_NV12, FRAMES_I420 = 0, 1, 2   # opk_frames.format (OPK_FRAMES_*)
_FORMAT_NAMES = {"nv12": FRAMES_NV12, "i420": FRAMES_I420}


def _frames_out(out, out_format, n, oh, ow, device):
    """The Frames destination of a render call, or None for the tensor path: `out` when it is a
    Frames, else fresh frames of out_format ("nv12" | "i420")."""
    if isinstance(out, Frames):
        assert out_format is None or _FORMAT_NAMES.get(out_format, out_format) == out.format
        return out
    if out_format is None:
        return None
    assert out is None, "out_format allocates the destination; pass a Frames as out instead"
    return Frames.empty(out_format, n, oh, ow, device)


class Frames:
    """A batch of frames as a decoder leaves it (opk_frames): packed BGR, NV12 (Y plane + interleaved
    UV plane) or I420 (Y, U and V planes), as uint8 CUDA tensors [n, rows, row bytes] -- rows may be
    padded (`width` pixels per row) and the frames any distance apart (tensor.stride(0)), so a
    view into the decoder's surfaces works without a copy.  Every method that takes `frames`
    accepts one; with NV12 / I420 it returns, bit for bit, what it returns on to_bgr()'s frames.
    The planes must stay alive and unchanged as the tensor form's frames must."""

    def __init__(self, fmt, planes, n, width, height):
        self.format, self.planes, self.n, self.width, self.height = fmt, planes, n, width, height

    @staticmethod
    def _plane(t, n, rows, row_bytes, what):
        assert t.dtype == torch.uint8 and t.is_cuda and t.dim() == 3, what + ": uint8 CUDA [n, rows, row bytes]"
        assert t.shape[0] == n and t.shape[1] == rows and t.shape[2] >= row_bytes, what + ": shape"
        assert t.stride(2) == 1 and (rows == 1 or t.stride(1) >= t.shape[2]), what + ": rows of bytes"
        return t

    @classmethod
    def nv12(cls, y, uv, width=None):
        """y [n, h, >= width], uv [n, h / 2, >= width] (U first); width default: y's row bytes."""
        n, h = y.shape[0], y.shape[1]
        w = y.shape[2] if width is None else width
        assert w % 2 == 0 and h % 2 == 0, "YUV 4:2:0 frames need an even width and height"
        return cls(FRAMES_NV12, [cls._plane(y, n, h, w, "y"), cls._plane(uv, n, h // 2, w, "uv")],
                   n, w, h)

    @classmethod
    def i420(cls, y, u, v, width=None):
        """y [n, h, >= width], u and v [n, h / 2, >= width / 2]; width default: y's row bytes."""
        n, h = y.shape[0], y.shape[1]
        w = y.shape[2] if width is None else width
        assert w % 2 == 0 and h % 2 == 0, "YUV 4:2:0 frames need an even width and height"
        return cls(FRAMES_I420, [cls._plane(y, n, h, w, "y"), cls._plane(u, n, h // 2, w // 2, "u"),
                                 cls._plane(v, n, h // 2, w // 2, "v")], n, w, h)

    @classmethod
    def bgr(cls, t, width=None):
        """t [n, h, w, 3], or [n, h, row bytes] with `width` pixels per row."""
        n, h, w, _ = _frame_rows(t, width)
        if t.dim() == 4:
            assert t.stride(3) == 1 and t.stride(2) == 3, "packed BGR pixels"
            t = t.as_strided((n, h, w * 3), (t.stride(0), t.stride(1), 1))
        return cls(FRAMES_BGR, [cls._plane(t, n, h, w * 3, "bgr")], n, w, h)

    @classmethod
    def empty_nv12(cls, n, h, w, device="cuda"):
        """Uninitialised NV12 frames to draw or convert into: y [n, h, w], uv [n, h / 2, w]."""
        assert w % 2 == 0 and h % 2 == 0, "YUV 4:2:0 frames need an even width and height"
        return cls.nv12(torch.empty((n, h, w), dtype=torch.uint8, device=device),
                        torch.empty((n, h // 2, w), dtype=torch.uint8, device=device))

    @classmethod
    def empty_i420(cls, n, h, w, device="cuda"):
        """Uninitialised I420 frames: y [n, h, w], u and v [n, h / 2, w / 2]."""
        assert w % 2 == 0 and h % 2 == 0, "YUV 4:2:0 frames need an even width and height"
        return cls.i420(torch.empty((n, h, w), dtype=torch.uint8, device=device),
                        torch.empty((n, h // 2, w // 2), dtype=torch.uint8, device=device),
                        torch.empty((n, h // 2, w // 2), dtype=torch.uint8, device=device))

    @classmethod
    def empty(cls, fmt, n, h, w, device="cuda"):
        """empty_nv12 / empty_i420 by name ("nv12" | "i420") or FRAMES_* value."""
        fmt = _FORMAT_NAMES.get(fmt, fmt)
        if fmt not in (FRAMES_NV12, FRAMES_I420):
            raise ValueError('out_format: "nv12" or "i420"')
        return (cls.empty_nv12 if fmt == FRAMES_NV12 else cls.empty_i420)(n, h, w, device)

    @classmethod
    def from_bgr(cls, ctx, t, fmt, out=None):
        """opk_bgr_to_frames: the BGR frames t ([n, h, w, 3] uint8 CUDA, or a BGR Frames) as NV12 or
        I420 (fmt "nv12" | "i420"), into the Frames `out` if given (then fmt may be None)."""
        src = t if isinstance(t, Frames) else cls.bgr(t)
        if out is None:
            out = cls.empty(fmt, src.n, src.height, src.width, src.device)
        s, d = src.struct(), out.struct_out()
        check(ctx.L.opk_bgr_to_frames(ctx.h, ctypes.byref(d), ctypes.byref(s)))
        return out

    @property
    def device(self):
        return self.planes[0].device

    def struct_out(self):
        """The opk_frames_out descriptor of these frames as a destination."""
        s, d = self.struct(), _lib.FramesOutStruct()
        ctypes.memmove(ctypes.byref(d), ctypes.byref(s), ctypes.sizeof(s))
        return d

    def struct(self):
        """The opk_frames descriptor (a _lib.FramesStruct; the planes stay owned by self)."""
        s = _lib.FramesStruct()
        s.format, s.n, s.width, s.height = self.format, self.n, self.width, self.height
        for i, t in enumerate(self.planes):
            s.plane[i] = t.data_ptr()
            # (a single row's stride says nothing; take it where it is a row step anyway)
            s.step[i] = t.stride(1) if t.shape[1] > 1 or t.stride(1) >= t.shape[2] else t.shape[2]
            s.frame_bytes[i] = t.stride(0) if self.n > 1 else 0
        return s

    def to_bgr(self, ctx, out=None):
        """opk_frames_to_bgr: the BGR frames uint8 [n, h, w, 3] (or into the rows of `out`, uint8
        [n, h, row bytes]) that every other method computes on."""
        if out is None:
            out = torch.empty((self.n, self.height, self.width, 3), dtype=torch.uint8,
                              device=self.device)
        s = self.struct()
        check(ctx.L.opk_frames_to_bgr(ctx.h, _ptr(out), _row_bytes(out, self.n, self.height, self.width),
                                      ctypes.byref(s)))
        return out


def _as_frames(frames, width=None, rows=False):
    """`frames` as a Frames: a Frames as it is; the tensor form -- uint8 [n, h, w, 3], with `rows`
    also [n, h, row bytes] of `width` pixels, a contiguous CUDA tensor -- as Frames.bgr of it."""
    if isinstance(frames, Frames):
        return frames
    if rows:
        _frame_rows(frames, width)
    else:
        n, h, w, c = frames.shape
        assert c == 3 and frames.dtype == torch.uint8
    _ptr(frames)
    return Frames.bgr(frames, width)


def jpeg_bound(n, width, height):
    """opk_jpeg_bound: a capacity that n JPEG files of width x height frames never exceed."""
    return int(_lib.load().opk_jpeg_bound(int(n), int(width), int(height)))


class JpegBatch:
    """The files of Context.encode_jpeg: frame f's file is data[offsets[f] : offsets[f + 1]].
    `data` (uint8 CUDA tensor, or numpy under host_only) stays on its side until asked for:
    .offsets (numpy uint64 [n + 1], one small download that waits for the encoder) and .sizes come
    first, .bytes(f) downloads one file, .tobytes_list() the batch in one copy."""

    def __init__(self, ctx, n, width, height, data, capacity, offsets_buf, host, source=None):
        self.ctx, self.n, self.width, self.height = ctx, n, width, height
        self.data, self.capacity, self.host = data, capacity, host
        self._offsets_buf, self._offsets = offsets_buf, None
        self._source = source   # the frames stay alive until the encoder has run

    @property
    def offsets(self):
        if self._offsets is None:
            if self.host:
                o = self._offsets_buf[:self.n + 1].copy()
            elif self.n == 0:
                o = np.zeros(1, np.uint64)   # no launch: nothing was written
            else:
                self.ctx.sync()
                o = self._offsets_buf[:self.n + 1].cpu().numpy().view(np.uint64)
            self._source = None
            if int(o[-1]) > self.capacity:
                raise OpkError("encode_jpeg: the files need %d bytes, the buffer holds %d"
                               % (int(o[-1]), self.capacity))
            self._offsets = o
        return self._offsets

    @property
    def sizes(self):
        return np.diff(self.offsets)

    def _download(self, lo, hi):
        part = self.data[lo:hi]
        return part.tobytes() if self.host else part.cpu().numpy().tobytes()

    def bytes(self, f):
        o = self.offsets
        return self._download(int(o[f]), int(o[f + 1]))

    def tobytes_list(self):
        o = self.offsets
        blob = self._download(0, int(o[-1]))
        return [blob[int(o[f]):int(o[f + 1])] for f in range(self.n)]

    def save(self, directory, names=None, first_index=None):
        """<directory>/<name>_rendered.jpg for each frame, as op::ImageSaver::saveImages names them;
        with first_index=k instead %012d_rendered.jpg from k on, op::VideoSaver's temporary frames.
        Returns the paths."""
        if (names is None) == (first_index is None):
            raise ValueError("names or first_index")
        if names is None:
            names = ["%012d" % (first_index + f) for f in range(self.n)]
        if len(names) != self.n:
            raise ValueError("%d names for %d frames" % (len(names), self.n))
        os.makedirs(directory, exist_ok=True)
        paths = []
        for name, blob in zip(names, self.tobytes_list()):
            paths.append(os.path.join(directory, "%s_rendered.jpg" % name))
            with open(paths[-1], "wb") as fh:
                fh.write(blob)
        return paths


# Handles still open at interpreter exit (e.g. held by a test traceback) are closed before the HIP
# runtime's own teardown: poses, then nets, then contexts.
_LIVE = {"pose": weakref.WeakSet(), "extractor": weakref.WeakSet(), "tracker": weakref.WeakSet(),
         "net": weakref.WeakSet(), "ctx": weakref.WeakSet()}


@atexit.register
def _close_live():
    for kind in ("pose", "extractor", "tracker", "net", "ctx"):
        for obj in list(_LIVE[kind]):
            try:
                obj.close()
            except Exception:
                pass


class dev_switches:
    """Context manager setting kernel-variant switches (opk_dev_set; A/B tests and tuning only),
    e.g. `with dev_switches(CONV3_W16=0): ...`; the product defaults are restored on exit."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        L = _lib.load()
        for k, v in self.kv.items():
            check(L.opk_dev_set(k.encode(), int(v), 0))
        return self

    def __exit__(self, *exc):
        L = _lib.load()
        for k in self.kv:
            L.opk_dev_set(k.encode(), 0, 1)
        return False


class launch_log:
    """Context manager over opk_launch_log_begin / _end: the [(layer, kernel)] list of every launch
    this thread makes inside the block, e.g. `with launch_log() as log: ...; [k for _, k in log]`
    (filled on exit; the layer is empty outside a net forward)."""

    def __enter__(self):
        self.lines = []
        check(_lib.load().opk_launch_log_begin())
        return self.lines

    def __exit__(self, *exc):
        L = _lib.load()
        need = ctypes.c_size_t()
        check(L.opk_launch_log_end(None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        check(L.opk_launch_log_end(buf, need.value, ctypes.byref(need)))
        self.lines.extend(tuple(line.split("\t", 1)) for line in buf.value.decode().splitlines())
        return False


class Context:
    """One opk_ctx bound to a device; runs on torch's current stream of that device."""

    def __init__(self, device=0, stream=None):
        self.L = _lib.load()
        self.device = device
        torch.cuda.set_device(device)
        s = stream if stream is not None else torch.cuda.current_stream(device)
        self.torch_stream = s
        h = ctypes.c_void_p()
        check(self.L.opk_ctx_create(device, ctypes.c_void_p(s.cuda_stream), ctypes.byref(h)))
        self.h = h
        _LIVE["ctx"].add(self)

    def close(self):
        if self.h:
            self.L.opk_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.L.opk_sync(self.h))

    @classmethod
    def host_only(cls):
        """A device-less context (-1): graph planning and conv listing only."""
        self = cls.__new__(cls)
        self.L = _lib.load()
        self.device = -1
        self.torch_stream = None
        h = ctypes.c_void_p()
        check(self.L.opk_ctx_create(-1, None, ctypes.byref(h)))
        self.h = h
        _LIVE["ctx"].add(self)
        return self

    def undistort_frames(self, frames, cameras, out=None):
        """opk_undistort_frames: the frames -- uint8 [n, h, w, 3] (CUDA) or a Frames (BGR, NV12,
        I420) -- undistorted, frame f through the maps of view f % V of `cameras` (a Cameras), as
        BGR uint8 [n, h, w, 3] (or into `out`: such a tensor, [n, h, row bytes], or a BGR Frames)."""
        src = _as_frames(frames)
        if out is None:
            out = torch.empty((src.n, src.height, src.width, 3), dtype=torch.uint8,
                              device=src.device)
        dst = out if isinstance(out, Frames) else Frames.bgr(out, src.width)
        s, d, c = src.struct(), dst.struct_out(), cameras.struct()
        check(self.L.opk_undistort_frames(self.h, ctypes.byref(d), ctypes.byref(s), ctypes.byref(c)))
        return out

    def orient_frames(self, frames, rotate=0, flip=False, out=None):
        """opk_orient_frames: the frames -- uint8 [n, h, w, 3] (CUDA) or a Frames (BGR, NV12, I420)
        -- rotated by `rotate` degrees (0, +-90, +-180, +-270) and mirrored if `flip`, as the
        reference's --frame_rotate / --frame_flip leave them, in their own format: a tensor
        [n, oh, ow, 3] for a tensor, a Frames for a Frames (or into `out`: such a tensor,
        [n, oh, row bytes], or a Frames of the format).  (ow, oh) = orient_size((w, h), rotate)."""
        src = _as_frames(frames)
        ow, oh = orient_size((src.width, src.height), rotate)
        if out is None:
            if isinstance(frames, Frames) and src.format != FRAMES_BGR:
                out = Frames.empty(src.format, src.n, oh, ow, src.device)
            else:
                out = torch.empty((src.n, oh, ow, 3), dtype=torch.uint8, device=src.device)
                if isinstance(frames, Frames):
                    out = Frames.bgr(out)
        dst = out if isinstance(out, Frames) else Frames.bgr(out, ow)
        s, d = src.struct(), dst.struct_out()
        check(self.L.opk_orient_frames(self.h, ctypes.byref(d), ctypes.byref(s), int(rotate),
                                       int(flip)))
        return out

    # ---- frames to JPEG files --------------------------------------------------------------------
    def encode_jpeg(self, frames, quality=100, out=None, capacity=None):
        """opk_jpeg_encode: the frames -- uint8 [n, h, w, 3] (CUDA) or a Frames (BGR, NV12, I420) --
        as baseline JPEG files, byte for byte what libjpeg writes for cv::imwrite's defaults at
        `quality` (the reference saves at 100), packed into one device buffer: a JpegBatch.
        Under host_only() the frames are a numpy uint8 [n, h, w, 3] (rows and frames may be
        strided) and opk_jpeg_encode_host runs.  The buffer holds jpeg_bound(n, w, h) bytes unless
        `capacity` says otherwise or `out` -- a JpegBatch of an earlier call, whose buffers are
        reused -- is given; files that do not fit raise OpkError naming the bytes needed."""
        host = self.device < 0
        if host:
            a = np.asarray(frames)
            assert a.dtype == np.uint8 and a.ndim == 4 and a.shape[3] == 3, "uint8 [n, h, w, 3]"
            n, h, w = a.shape[:3]
            if n and h and w and (a.strides[3] != 1 or a.strides[2] != 3 or a.strides[1] < 3 * w
                                  or (n > 1 and a.strides[0] <= 0)):
                a = np.ascontiguousarray(a)
            src = a
        else:
            src = _as_frames(frames)
            n, h, w = src.n, src.height, src.width
        if out is not None:
            assert isinstance(out, JpegBatch) and out.host == host and capacity is None
            data, cap = out.data, out.capacity
            offsets = out._offsets_buf if out._offsets_buf.shape[0] >= n + 1 else None
        else:
            cap = jpeg_bound(n, w, h) if capacity is None else int(capacity)
            data, offsets = None, None
        if host:
            if data is None:
                data = np.empty(max(cap, 1), np.uint8)
            if offsets is None:
                offsets = np.zeros(n + 1, np.uint64)
            step, frame = (a.strides[1], a.strides[0]) if n and h and w else (0, 0)
            check(self.L.opk_jpeg_encode_host(
                data.ctypes.data_as(ctypes.c_void_p), cap, offsets.ctypes.data_as(ctypes.c_void_p),
                a.ctypes.data_as(ctypes.c_void_p), step, frame if n > 1 else 0, n, w, h, int(quality)))
        else:
            if data is None:
                data = torch.empty(max(cap, 1), dtype=torch.uint8, device=src.device)
            if offsets is None:
                offsets = torch.zeros(n + 1, dtype=torch.int64, device=src.device)
            s = src.struct()
            check(self.L.opk_jpeg_encode(self.h, _ptr(data), cap, _ptr(offsets), ctypes.byref(s),
                                         int(quality)))
        batch = JpegBatch(self, n, w, h, data, cap, offsets, host, src)
        if cap < jpeg_bound(n, w, h):
            batch.offsets   # may not fit: look now
        return batch

    # ---- person ids across frames -------------------------------------------------------------
    def pyramid(self, frames, levels=3):
        """opk_pyramid_build: the grey image and Gaussian pyramid (`levels` 1..3) of every frame --
        uint8 [n, h, w, 3] BGR (CUDA) or a Frames (BGR, NV12, I420) -- as a Pyramid."""
        fr = frames if isinstance(frames, Frames) else Frames.bgr(frames)
        pyr = Pyramid(self, fr.n, fr.width, fr.height, levels, fr.device)
        s = fr.struct()
        check(self.L.opk_pyramid_build(self.h, _ptr(pyr.buffer), ctypes.byref(s), levels))
        return pyr

    def lk_points(self, pyramid, points, carry=None):
        """opk_lk_points: one pyramidal Lucas-Kanade launch over `points`, a numpy array of LK_POINT
        records (frame_i, frame_j, x, y, status) addressing the frames of `pyramid` (3 levels) and,
        as frame -1, the single frame of the Pyramid `carry`.  Returns the updated records."""
        pts = np.ascontiguousarray(points, LK_POINT)
        if carry is not None:
            assert (carry.n, carry.width, carry.height, carry.levels) == (
                1, pyramid.width, pyramid.height, pyramid.levels)
        dev = torch.from_numpy(pts.view(np.uint8).reshape(-1).copy()).to(pyramid.buffer.device)
        check(self.L.opk_lk_points(self.h, _ptr(pyramid.buffer), pyramid.n,
                                   _ptr(carry.buffer) if carry is not None else None,
                                   pyramid.width, pyramid.height, _ptr(dev) if pts.size else None,
                                   pts.size))
        self.sync()
        return dev.cpu().numpy().view(LK_POINT).reshape(pts.shape)

    # ---- operators ---------------------------------------------------------------------------
    def convert(self, dst, src):
        """dst <- src element-wise on the device (float32 <-> float64, opk_convert), same count."""
        kinds = {torch.float32: 0, torch.float64: 1}
        assert dst.numel() == src.numel() and dst.dtype in kinds and src.dtype in kinds
        assert dst.is_contiguous() and src.is_contiguous()
        check(self.L.opk_convert(self.h, _ptr(dst), kinds[dst.dtype], _ptr(src), kinds[src.dtype],
                                 src.numel()))

    def resize_and_merge(self, target, sources, semantics=MAPS_CPU, scale_ratios=None):
        """target [N,C,H,W] fp32 CUDA; sources list of [N,C,h,w] (resizeAndMergeGpu).  semantics
        MAPS_CPU: resizeAndMergeCpu's arithmetic; MAPS_CUDA: the CUDA build's (scale_ratios =
        scaleInputToNetInputs, needed with several sources)."""
        n = len(sources)
        ptrs = (ctypes.c_void_p * n)(*[s.data_ptr() for s in sources])
        sizes = (ctypes.c_int * (4 * n))(*[int(v) for s in sources for v in s.shape])
        ratios = None if scale_ratios is None else (ctypes.c_float * n)(*[float(r) for r in scale_ratios])
        check(self.L.opk_resize_and_merge_semantics(self.h, _ptr(target), ptrs, n,
                                                    int4(target.shape), sizes, ratios, semantics))

    def cvmat_to_input(self, net_input, frames, scale, normalize=1, width=None):
        """op::CvMatToOpInput for one scale: frames [n, h, w, 3] uint8 BGR (CUDA) ->
        net_input [n, 3, net_h, net_w] float32 (CUDA).  Frames with padded rows (a cv::Mat step)
        come as [n, h, row bytes] with `width` pixels per row; the frames may be a view that
        starts anywhere in a larger contiguous buffer (any base alignment).  Or a Frames."""
        frames = _as_frames(frames, width, rows=True)
        assert net_input.shape[0] == frames.n and net_input.shape[1] == 3
        s = frames.struct()
        check(self.L.opk_cvmat_to_input_fmt(self.h, _ptr(net_input), ctypes.byref(s), float(scale),
                                            net_input.shape[3], net_input.shape[2], normalize))

    def nms(self, peaks, heat, threshold=NMS_THRESHOLD, offset=(0.0, 0.0), semantics=MAPS_CPU):
        """peaks [N,parts,maxPeaks+1,3]; heat [N,C,H,W] (nmsGpu; semantics MAPS_CPU: nmsCpu's
        rules, MAPS_CUDA: nmsGpu's)."""
        check(self.L.opk_nms_semantics(self.h, _ptr(peaks), None, _ptr(heat), threshold,
                                       int4(peaks.shape), int4(heat.shape), offset[0], offset[1],
                                       semantics))

    def probe_peaks(self):
        """Measured ceilings on this device (opk_probe_peaks): dense fp16 MFMA TFLOP/s on random
        and on zero operands, streaming HBM read GB/s."""
        r, z, h = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(self.L.opk_probe_peaks(self.h, ctypes.byref(r), ctypes.byref(z), ctypes.byref(h)))
        return {"mfma_fp16_random_tflops": round(r.value, 1), "mfma_fp16_zero_tflops": round(z.value, 1),
                "hbm_read_gbs": round(h.value, 1)}

    # ---- renderers (renderPose.cu / renderFace.cu / renderHand.cu) ---------------------------
    # frame: float32 CUDA [h, w, 3] BGR, drawn in place; keypoints float32 CUDA [people, parts, 3]
    def render_pose_keypoints(self, frame, pose, pose_model=BODY_25, threshold=0.05,
                              googly_eyes=False, blend_original=True, alpha=0.6):
        """op::renderPoseKeypointsGpu (POSE_DEFAULT_ALPHA_KEYPOINT 0.6)."""
        h, w = frame.shape[:2]
        people = 0 if pose is None else pose.shape[0]
        check(self.L.opk_render_pose_keypoints(self.h, _ptr(frame), pose_model, people, w, h,
                                               None if pose is None else _ptr(pose), threshold,
                                               int(googly_eyes), int(blend_original), alpha))

    def render_face_keypoints(self, frame, face, threshold=0.4, alpha=0.6):
        """op::renderFaceKeypointsGpu; face [people, 70, 3]."""
        h, w = frame.shape[:2]
        check(self.L.opk_render_face_keypoints(self.h, _ptr(frame), w, h, _ptr(face), face.shape[0],
                                               threshold, alpha))

    def render_hand_keypoints(self, frame, hands, threshold=0.2, alpha=0.6):
        """op::renderHandKeypointsGpu; hands [n, 21, 3]."""
        h, w = frame.shape[:2]
        check(self.L.opk_render_hand_keypoints(self.h, _ptr(frame), w, h, _ptr(hands),
                                               hands.shape[0], threshold, alpha))

    def render_heat_map(self, frame, heat, scale, part, alpha=0.7, distance=False):
        """op::renderPoseHeatMapGpu (distance: op::renderPoseDistanceGpu); heat [C, hh, hw]."""
        h, w = frame.shape[:2]
        fn = self.L.opk_render_pose_distance if distance else self.L.opk_render_pose_heat_map
        check(fn(self.h, _ptr(frame), w, h, _ptr(heat), heat.shape[-1], heat.shape[-2], scale,
                 part, alpha))

    def render_heat_maps(self, frame, heat, scale, pose_model=BODY_25, alpha=0.7):
        """op::renderPoseHeatMapsGpu."""
        h, w = frame.shape[:2]
        check(self.L.opk_render_pose_heat_maps(self.h, _ptr(frame), pose_model, w, h, _ptr(heat),
                                               heat.shape[-1], heat.shape[-2], scale, alpha))

    def render_pafs(self, frame, heat, scale, part=None, pose_model=BODY_25, alpha=0.7):
        """op::renderPosePAFGpu (part = its x channel) or, part None, op::renderPosePAFsGpu."""
        h, w = frame.shape[:2]
        if part is None:
            check(self.L.opk_render_pose_pafs(self.h, _ptr(frame), pose_model, w, h, _ptr(heat),
                                              heat.shape[-1], heat.shape[-2], scale, alpha))
        else:
            check(self.L.opk_render_pose_paf(self.h, _ptr(frame), pose_model, w, h, _ptr(heat),
                                             heat.shape[-1], heat.shape[-2], scale, part, alpha))

    # ---- the output image (CvMatToOpOutput / OpOutputToCvMat) and the fused batch render --------
    def cvmat_to_output(self, frames, scale=1.0, out_size=None):
        """op::CvMatToOpOutput for a batch: frames [n, h, w, 3] uint8 BGR (CUDA) -> float32
        [n, out_h, out_w, 3]; out_size = (w, h), default the frames' own.  Or a Frames."""
        frames = _as_frames(frames)
        ow, oh = out_size if out_size is not None else (frames.width, frames.height)
        out = torch.empty((frames.n, max(oh, 0), max(ow, 0), 3), dtype=torch.float32,
                          device=frames.device)
        s = frames.struct()
        check(self.L.opk_cvmat_to_output_fmt(self.h, _ptr(out), ctypes.byref(s), float(scale), ow, oh))
        return out

    def output_to_cvmat(self, output, cast=CAST_CPU, out=None):
        """op::OpOutputToCvMat for a batch: float32 [n, h, w, 3] -> uint8 [n, h, w, 3] (or into the
        rows of `out`, uint8 [n, h, row bytes >= w*3])."""
        n, h, w, c = output.shape
        assert c == 3 and output.dtype == torch.float32
        if out is None:
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=output.device)
        check(self.L.opk_output_to_cvmat(self.h, _ptr(out), _row_bytes(out, n, h, w), _ptr(output),
                                         n, w, h, cast))
        return out

    def render_frames(self, frames, layers, scale=1.0, out_size=None, blend_original=True,
                      cast=CAST_CPU, out=None, heat=None, out_format=None):
        """CvMatToOpOutput -> the heat layer (a RenderHeat), if any -> the keypoint layers in
        order -> OpOutputToCvMat in one kernel: frames [n, h, w, 3] uint8 BGR (CUDA), layers a
        list of RenderLayer -> uint8 [n, out_h, out_w, 3] (or into the rows of `out`, uint8
        [n, out_h, row bytes]).  frames may be a Frames (BGR, NV12 or I420).
        Frames out: with a Frames as `out` (BGR, NV12 or I420), or out_format="nv12" | "i420",
        the drawn frames go there (opk_render_frames_to: Frames.from_bgr of the tensor result, bit
        for bit, converted inside the render) and that Frames is returned."""
        frames = _as_frames(frames)
        fs, n = frames.struct(), frames.n
        ow, oh = out_size if out_size is not None else (frames.width, frames.height)
        dest = _frames_out(out, out_format, n, oh, ow, frames.device)
        if dest is None and out is None:
            out = torch.empty((n, max(oh, 0), max(ow, 0), 3), dtype=torch.uint8,
                              device=frames.device)
        arr = (_lib.RenderLayerStruct * max(len(layers), 1))()
        keep = []
        for s, l in zip(arr, layers):
            assert len(l.counts) == n, "one count per frame"
            counts = (ctypes.c_int * max(n, 1))(*[int(v) for v in l.counts])
            keep.append(counts)
            parts = {LAYER_FACE: 70, LAYER_HAND: 21}.get(l.kind)
            if parts is None and l.kind == LAYER_POSE and 0 <= l.pose_model <= 14:
                parts = pose_model_info(l.pose_model)["parts"]
            if l.keypoints is None:
                assert sum(l.counts) == 0, "keypoints missing"
            elif parts is not None:   # (an unknown kind or model is the library's error)
                assert l.keypoints.dtype == torch.float32
                assert tuple(l.keypoints.shape) == (sum(l.counts), parts, 3), "keypoints shape"
            s.kind, s.pose_model = l.kind, l.pose_model
            s.keypoints_dev = None if l.keypoints is None else _ptr(l.keypoints)
            s.counts_host = counts
            s.render_threshold, s.alpha, s.googly_eyes = l.threshold, l.alpha, int(l.googly_eyes)
        hs = None if heat is None else ctypes.byref(self._heat_struct(heat, n))
        if dest is not None:
            ds = dest.struct_out()
            check(self.L.opk_render_frames_to(self.h, ctypes.byref(ds), ctypes.byref(fs),
                                              float(scale), arr, len(layers), int(blend_original),
                                              cast, hs))
            return dest
        # (not through _to: that refuses a destination that overlaps its source; this form does not)
        check(self.L.opk_render_frames_heat_fmt(self.h, _ptr(out), _row_bytes(out, n, oh, ow), ow,
                                                oh, ctypes.byref(fs), float(scale), arr, len(layers),
                                                int(blend_original), cast, hs))
        return out

    @staticmethod
    def _heat_struct(heat, n):
        """opk_render_heat of a RenderHeat on n frames."""
        hs = _lib.RenderHeatStruct()
        hs.kind, hs.pose_model, hs.channel = heat.kind, heat.pose_model, heat.channel
        if heat.heat is not None:
            assert heat.heat.dtype == torch.float32 and heat.heat.dim() == 4
            assert heat.heat.shape[0] == n, "one heat stack per frame"
            hs.heat_dev = _ptr(heat.heat)
            hs.channels, hs.heat_h, hs.heat_w = heat.heat.shape[1:]
        hs.scale_to_keep_ratio, hs.alpha = heat.scale, heat.alpha
        return hs

    def paf_scores(self, scores, heat, peaks, pose_model=BODY_25, inter_th=CONNECT_INTER_THRESHOLD,
                   inter_min_above=CONNECT_INTER_MIN_ABOVE_THRESHOLD, nms_th=NMS_THRESHOLD):
        n, c, h, w = heat.shape
        check(self.L.opk_paf_scores(self.h, _ptr(scores), _ptr(heat), _ptr(peaks), n, pose_model, c,
                                    h, w, peaks.shape[2] - 1, inter_th, inter_min_above, nms_th))

    def paf_scores_sources(self, out, sources, target_hw, peaks, pose_model=BODY_25,
                           inter_th=CONNECT_INTER_THRESHOLD,
                           inter_min_above=CONNECT_INTER_MIN_ABOVE_THRESHOLD, nms_th=NMS_THRESHOLD,
                           semantics=MAPS_CPU, scale_ratios=None, rec_floats=0):
        """The pipeline's PAF scorer on its lazy heat map (opk_paf_scores_sources): sources a list
        of [N, C, h, w] net outputs resized to target_hw = (H, W) and averaged on the fly; peaks
        [N, parts, maxPeaks+1, 3].  rec_floats 0: out is the dense [N, pairs, maxPeaks, maxPeaks]
        array; else out is [N, rec_floats], one compact record per frame.  Returns the bytes of
        the sources a workgroup stages on chip (0: read from memory)."""
        n = len(sources)
        ptrs = (ctypes.c_void_p * n)(*[_ptr(s).value for s in sources])
        sizes = (ctypes.c_int * (4 * n))(*[int(v) for s in sources for v in s.shape])
        ratios = None if scale_ratios is None else (ctypes.c_float * n)(*[float(r) for r in scale_ratios])
        assert peaks.shape[0] == sources[0].shape[0] and peaks.dtype == torch.float32
        assert out.dtype == torch.float32 and all(s.dtype == torch.float32 for s in sources)
        assert rec_floats == 0 or out.numel() == peaks.shape[0] * rec_floats
        staged = ctypes.c_size_t()
        check(self.L.opk_paf_scores_sources(self.h, _ptr(out), rec_floats, ptrs, n, sizes,
                                            target_hw[0], target_hw[1], semantics, ratios,
                                            _ptr(peaks), pose_model, peaks.shape[2] - 1, inter_th,
                                            inter_min_above, nms_th, ctypes.byref(staged)))
        return staged.value

    def connect_body_parts(self, heat, peaks, pose_model=BODY_25, scale=1.0, max_people=512,
                           inter_min_above=CONNECT_INTER_MIN_ABOVE_THRESHOLD,
                           inter_th=CONNECT_INTER_THRESHOLD, min_subset_cnt=CONNECT_MIN_SUBSET_CNT,
                           min_subset_score=CONNECT_MIN_SUBSET_SCORE, nms_th=NMS_THRESHOLD,
                           maximize_positives=False, semantics=CONNECT_CPU):
        """One frame: heat [C,H,W] / [1,C,H,W], peaks [parts,maxPeaks+1,3] (connectBodyPartsGpu
        replacement; semantics CONNECT_CPU / CONNECT_GPU picks the people assembly)."""
        c, h, w = heat.shape[-3:]
        parts = peaks.shape[-3]
        kp = np.zeros((max_people, parts, 3), np.float32)
        ks = np.zeros(max_people, np.float32)
        n = ctypes.c_int()
        check(self.L.opk_connect_body_parts_semantics(
            self.h, kp.ctypes.data_as(ctypes.c_void_p), ks.ctypes.data_as(ctypes.c_void_p),
            max_people, ctypes.byref(n), _ptr(heat), _ptr(peaks), pose_model, c, h, w,
            peaks.shape[-2] - 1, inter_min_above, inter_th, min_subset_cnt, min_subset_score,
            nms_th, scale, int(maximize_positives), semantics))
        k = min(n.value, max_people)
        return kp[:k].copy(), ks[:k].copy()


def orient_size(size, rotate):
    """opk_orient_size: (width, height) of frames of `size` rotated by `rotate` degrees."""
    w, h = ctypes.c_int(), ctypes.c_int()
    check(_lib.load().opk_orient_size(int(size[0]), int(size[1]), int(rotate), ctypes.byref(w),
                                      ctypes.byref(h)))
    return w.value, h.value


def orient_keypoints(keypoints, size, rotate, flip, inverse=False):
    """opk_orient_keypoints: a copy of keypoints [people, parts, 3] taken from the coordinates of
    the source frames (`size`, their (width, height)) to those of the oriented frames, or back with
    `inverse`; points whose third value is 0 stay as they are."""
    kp = np.array(keypoints, dtype=np.float32, order="C")
    assert kp.ndim == 3 and kp.shape[2] == 3
    check(_lib.load().opk_orient_keypoints(kp.ctypes.data_as(ctypes.c_void_p), kp.shape[0],
                                           kp.shape[1], int(size[0]), int(size[1]), int(rotate),
                                           int(flip), int(inverse)))
    return kp


def scale_and_size(input_size, net_resolution=(-1, 368), dynamic_behavior=1.0, scale_number=1,
                   scale_gap=0.25):
    """op::ScaleAndSizeExtractor::extract: ([scaleInputToNetInputs], [(net_w, net_h)])."""
    L = _lib.load()
    scales = (ctypes.c_double * scale_number)()
    sizes = (ctypes.c_int * (2 * scale_number))()
    check(L.opk_scale_and_size(input_size[0], input_size[1], net_resolution[0], net_resolution[1],
                               float(dynamic_behavior), scale_number, float(scale_gap), scales,
                               sizes))
    return list(scales), [(sizes[2 * i], sizes[2 * i + 1]) for i in range(scale_number)]


def scale_keypoints(keypoints, scale_mode, scale_input_to_output=1.0, scale_net_to_output=1.0,
                    producer_size=(1, 1)):
    """op::KeypointScaler::scale on a copy of keypoints [people, parts, 3]."""
    kp = np.ascontiguousarray(keypoints, np.float32).copy()
    check(_lib.load().opk_scale_keypoints(kp.ctypes.data_as(ctypes.c_void_p), kp.shape[0],
                                          kp.shape[1], scale_mode, float(scale_input_to_output),
                                          float(scale_net_to_output), producer_size[0],
                                          producer_size[1]))
    return kp


def keep_top_n_people(keypoints, scores, max_people):
    """op::KeepTopNPeople::keepTopPeople: (kept keypoints, source index of each kept row)."""
    kp = np.ascontiguousarray(keypoints, np.float32)
    sc = np.ascontiguousarray(scores, np.float32)
    rows = max(kp.shape[0], max_people, 1)
    out = np.zeros((rows,) + kp.shape[1:], np.float32)
    idx = np.full(rows, -1, np.int32)
    n = ctypes.c_int()
    check(_lib.load().opk_keep_top_n_people(kp.ctypes.data_as(ctypes.c_void_p), kp.shape[0],
                                            kp.shape[1], sc.ctypes.data_as(ctypes.c_void_p),
                                            max_people, out.ctypes.data_as(ctypes.c_void_p),
                                            idx.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)))
    return out[:n.value], idx[:n.value]


class _JsonKeypoints(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("ndims", ctypes.c_int),
                ("people", ctypes.c_int), ("parts", ctypes.c_int), ("dims", ctypes.c_int)]


def _json_args(keypoint_vector, candidates):
    keep = []
    arr = (_JsonKeypoints * max(len(keypoint_vector), 1))()
    for i, (a, name) in enumerate(keypoint_vector):
        a = np.ascontiguousarray(a if a is not None else np.zeros(0), np.float32)
        keep.append(a)
        shape = a.shape if a.size else ()
        if len(shape) not in (0, 1, 3):
            shape = (None,) * 2   # rejected by the library like the reference
        dims = list(shape) + [0] * (3 - len(shape))
        arr[i] = _JsonKeypoints(name.encode(), a.ctypes.data if a.size else None, len(shape),
                                dims[0] or 0, dims[1] or 0, dims[2] or 0)
    cands = candidates or []
    counts = np.array([len(c) for c in cands], np.int32)
    flat = np.ascontiguousarray(
        np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in cands])
        if cands and counts.sum() else np.zeros((0, 3)), np.float32)
    keep += [counts, flat]
    return arr, keep, (flat.ctypes.data if flat.size else None,
                       counts.ctypes.data if counts.size else None, len(cands))


def people_json(keypoint_vector, candidates=None, human_readable=False):
    """op::savePeopleJson's file text (fileStream.cpp:306-344) for keypoint_vector = [(array, name)]
    (arrays [people][parts][3], [people] or empty) and candidates = per-part lists of [x, y, score]."""
    L = _lib.load()
    arr, keep, (cp, cc, nparts) = _json_args(keypoint_vector, candidates)
    n = ctypes.c_size_t()
    check(L.opk_people_json(arr, len(keypoint_vector), cp, cc, nparts, int(human_readable), None,
                            0, ctypes.byref(n)))
    buf = ctypes.create_string_buffer(n.value + 1)
    check(L.opk_people_json(arr, len(keypoint_vector), cp, cc, nparts, int(human_readable), buf,
                            n.value + 1, ctypes.byref(n)))
    del keep
    return buf.raw[:n.value].decode()


def save_people_json(path, keypoint_vector, candidates=None, human_readable=False):
    """PeopleJsonSaver::save (peopleJsonSaver.cpp:15-30): the same text written to path."""
    L = _lib.load()
    arr, keep, (cp, cc, nparts) = _json_args(keypoint_vector, candidates)
    check(L.opk_save_people_json(path.encode(), arr, len(keypoint_vector), cp, cc, nparts,
                                 int(human_readable)))
    del keep


def datum_keypoint_vector(pose_keypoints, face_keypoints=None, hand_keypoints=(None, None),
                          person_ids=None, pose_keypoints_3d=None, face_keypoints_3d=None,
                          hand_keypoints_3d=(None, None)):
    """The keypointVector WPeopleJsonSaver builds from a Datum (wPeopleJsonSaver.hpp:75-88):
    person ids (-1 each without a person-id extractor, PoseExtractor::extractIds,
    poseExtractor.cpp:136-151; person_ids: a Tracker's), the 2-D body / face / hand arrays and the
    3-D ones ([1, parts, 4] of a rig's time step, PoseExtractor.keypoints_3d; empty without)."""
    pk = np.asarray(pose_keypoints, np.float32)
    ids = np.full(pk.shape[0], -1, np.float32) if pk.size else None
    if person_ids is not None and pk.size:
        ids = np.asarray(person_ids, np.float32)
    return [(ids, "person_id"), (pk, "pose_keypoints_2d"), (face_keypoints, "face_keypoints_2d"),
            (hand_keypoints[0], "hand_left_keypoints_2d"),
            (hand_keypoints[1], "hand_right_keypoints_2d"),
            (pose_keypoints_3d, "pose_keypoints_3d"), (face_keypoints_3d, "face_keypoints_3d"),
            (hand_keypoints_3d[0], "hand_left_keypoints_3d"),
            (hand_keypoints_3d[1], "hand_right_keypoints_3d")]


def caffemodel_blob(path, layer, index):
    """Host utility: (shape, float32 data) of a blob in a .caffemodel (opk_caffemodel_blob)."""
    L = _lib.load()
    shape = (ctypes.c_int64 * 8)()
    nd = ctypes.c_int()
    check(L.opk_caffemodel_blob(path.encode(), layer.encode(), index, None, 0, shape,
                                ctypes.byref(nd)))
    dims = tuple(shape[i] for i in range(nd.value))
    out = np.empty(int(np.prod(dims)) if dims else 0, np.float32)
    check(L.opk_caffemodel_blob(path.encode(), layer.encode(), index,
                                out.ctypes.data_as(ctypes.c_void_p), out.size, shape,
                                ctypes.byref(nd)))
    return dims, out.reshape(dims)


def pose_model_info(pose_model):
    """Tables of a PoseModel from libopk_hip: dict(parts, bkg, pairs, map_idx, heat_channels,
    nms_threshold, inter_threshold)."""
    L = _lib.load()
    parts, bkg, npairs, hc = (ctypes.c_int() for _ in range(4))
    check(L.opk_pose_model_info(pose_model, ctypes.byref(parts), ctypes.byref(bkg),
                                ctypes.byref(npairs), ctypes.byref(hc), None, None))
    pairs = np.zeros(2 * npairs.value, np.int32)
    nmap = hc.value - parts.value - bkg.value
    mi = np.zeros(max(nmap, 1), np.int32)
    check(L.opk_pose_model_info(pose_model, None, None, None, None,
                                pairs.ctypes.data_as(ctypes.c_void_p),
                                mi.ctypes.data_as(ctypes.c_void_p)))
    nms, inter = ctypes.c_float(), ctypes.c_float()
    check(L.opk_pose_default_thresholds(pose_model, 0, ctypes.byref(nms), ctypes.byref(inter)))
    return dict(id=pose_model, parts=parts.value, bkg=bool(bkg.value), pairs=pairs.tolist(),
                map_idx=mi[:nmap].tolist(), heat_channels=hc.value, nms_threshold=nms.value,
                inter_threshold=inter.value)


def assemble_people(pair_scores, peaks, pose_model=BODY_25, scale=1.0, max_people=512,
                    min_subset_cnt=CONNECT_MIN_SUBSET_CNT, min_subset_score=CONNECT_MIN_SUBSET_SCORE,
                    maximize_positives=False, semantics=CONNECT_CPU):
    """Host-only assembly from numpy pair scores [npairs,mp,mp] + peaks [parts,mp+1,3]."""
    L = _lib.load()
    pair_scores = np.ascontiguousarray(pair_scores, np.float32)
    peaks = np.ascontiguousarray(peaks, np.float32)
    parts = peaks.shape[0]
    kp = np.zeros((max_people, parts, 3), np.float32)
    ks = np.zeros(max_people, np.float32)
    n = ctypes.c_int()
    check(L.opk_assemble_people_semantics(kp.ctypes.data_as(ctypes.c_void_p),
                                          ks.ctypes.data_as(ctypes.c_void_p), max_people,
                                          ctypes.byref(n),
                                          pair_scores.ctypes.data_as(ctypes.c_void_p),
                                          peaks.ctypes.data_as(ctypes.c_void_p), pose_model,
                                          peaks.shape[1] - 1, min_subset_cnt, min_subset_score,
                                          scale, int(maximize_positives), semantics))
    k = min(n.value, max_people)
    return kp[:k].copy(), ks[:k].copy()


# opk_lk_point: one point of Context.lk_points
LK_POINT = np.dtype([("frame_i", "<i4"), ("frame_j", "<i4"), ("x", "<f4"), ("y", "<f4"),
                     ("status", "<i4")])
# op::PersonIdExtractor's defaults (personIdExtractor.hpp:11-12)
TRACK_CONFIDENCE, TRACK_INLIER_RATIO, TRACK_DISTANCE, TRACK_FRAMES_TO_DELETE = 0.1, 0.5, 30.0, 10


def pyramid_layout(width, height, levels=3):
    """opk_pyramid_layout: dict(sizes=[(w, h)] per level, offsets=[bytes], frame_bytes) of one
    frame's pyramid record (level 0 uint8, level 1 uint16 = 256 x value, level 2 float32)."""
    n = max(levels, 1)
    w, h = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    at, fb = (ctypes.c_size_t * n)(), ctypes.c_size_t()
    check(_lib.load().opk_pyramid_layout(width, height, levels, w, h, at, ctypes.byref(fb)))
    return dict(sizes=[(w[i], h[i]) for i in range(levels)], offsets=[at[i] for i in range(levels)],
                frame_bytes=fb.value)


class Pyramid:
    """The pyramid records of n frames on the device (Context.pyramid)."""

    def __init__(self, ctx, n, width, height, levels, device="cuda", buffer=None):
        self.ctx, self.n, self.width, self.height, self.levels = ctx, n, width, height, levels
        self.layout = pyramid_layout(width, height, levels)
        fb = self.layout["frame_bytes"]
        self.buffer = buffer if buffer is not None else torch.empty(max(n * fb, 1), dtype=torch.uint8,
                                                                    device=device)

    def frame(self, f):
        """The record of frame f as a one-frame Pyramid sharing this buffer (a carry frame)."""
        fb = self.layout["frame_bytes"]
        return Pyramid(self.ctx, 1, self.width, self.height, self.levels,
                       buffer=self.buffer[f * fb:(f + 1) * fb])

    def level(self, level):
        """opk_pyramid_level: float32 numpy [n, h, w] of one level."""
        w, h = self.layout["sizes"][level] if 0 <= level < self.levels else (1, 1)
        out = torch.empty((self.n, h, w), dtype=torch.float32, device=self.buffer.device)
        check(self.ctx.L.opk_pyramid_level(self.ctx.h, _ptr(out), _ptr(self.buffer), self.n,
                                           self.width, self.height, self.levels, level))
        self.ctx.sync()
        return out.cpu().numpy()


def match_people(entries, entry_ids, people, size, next_id=0, inlier_ratio=TRACK_INLIER_RATIO,
                 distance=TRACK_DISTANCE):
    """opk_match_people (matchLKAndOPGreedy; host only): entries [n, parts, 3] and people
    [m, parts, 3] of (x, y, status), entry_ids ascending, size = (width, height).  Returns
    (ids int64 [m], next_id)."""
    people = np.ascontiguousarray(people, np.float32)
    entries = np.ascontiguousarray(entries, np.float32).reshape(-1, *people.shape[1:])
    eid = np.ascontiguousarray(entry_ids, np.int64)
    assert eid.shape == (entries.shape[0],) and people.ndim == 3 and people.shape[2] == 3
    ids = np.full(people.shape[0], -2, np.int64)
    nid = ctypes.c_longlong(next_id)
    check(_lib.load().opk_match_people(
        entries.ctypes.data_as(ctypes.c_void_p), eid.ctypes.data_as(ctypes.c_void_p),
        entries.shape[0], people.ctypes.data_as(ctypes.c_void_p), people.shape[0], people.shape[1],
        inlier_ratio, distance, size[0], size[1], ctypes.byref(nid),
        ids.ctypes.data_as(ctypes.c_void_p)))
    return ids, nid.value


class Tracker:
    """Person ids across video frames (op::PersonIdExtractor, --identification): a 3-level pyramid
    per frame, one Lucas-Kanade step per level around every keypoint of the tracked people, and the
    reference's greedy match of the propagated people against the new detections."""

    def __init__(self, ctx, confidence=TRACK_CONFIDENCE, inlier_ratio=TRACK_INLIER_RATIO,
                 distance=TRACK_DISTANCE, frames_to_delete=TRACK_FRAMES_TO_DELETE):
        self.ctx, self.L = ctx, ctx.L
        h = ctypes.c_void_p()
        check(self.L.opk_tracker_create(ctx.h, confidence, inlier_ratio, distance, frames_to_delete,
                                        ctypes.byref(h)))
        self.h = h
        _LIVE["tracker"].add(self)

    def close(self):
        if self.h:
            self.L.opk_tracker_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(self.L.opk_tracker_reset(self.h))

    def update(self, frames, keypoints_list):
        """The ids of the people of n consecutive frames: frames uint8 [n, h, w, 3] BGR (CUDA) or a
        Frames; keypoints_list = per frame [people, parts, 3] (x, y, score).  Returns a list of
        int64 arrays.  Any number of calls; the state carries over."""
        fr = frames if isinstance(frames, Frames) else Frames.bgr(frames)
        assert len(keypoints_list) == fr.n
        kps = [np.ascontiguousarray(k, np.float32) for k in keypoints_list]
        parts = max([k.shape[1] for k in kps if k.ndim == 3] + [1])
        kps = [k.reshape(-1, parts, 3) for k in kps]
        counts = np.array([k.shape[0] for k in kps], np.int32)
        flat = np.ascontiguousarray(np.concatenate(kps) if kps else np.zeros((0, parts, 3), np.float32))
        ids = np.full(int(counts.sum()), -2, np.int64)
        s = fr.struct()
        check(self.L.opk_tracker_update(self.h, ctypes.byref(s),
                                        flat.ctypes.data_as(ctypes.c_void_p),
                                        counts.ctypes.data_as(ctypes.c_void_p), parts,
                                        ids.ctypes.data_as(ctypes.c_void_p)))
        return [a.copy() for a in np.split(ids, np.cumsum(counts)[:-1])] if fr.n else []

    def set_timing(self, on=True):
        check(self.L.opk_tracker_set_timing(self.h, int(on)))

    def read_times(self):
        """{batches, pyramid_ms, lk_ms, host_ms, device_bytes} since the last read."""
        b, p, l, h = ctypes.c_int(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        m = ctypes.c_size_t(0)
        check(self.L.opk_tracker_read_times(self.h, ctypes.byref(b), ctypes.byref(p), ctypes.byref(l),
                                            ctypes.byref(h), ctypes.byref(m)))
        return {"batches": b.value, "pyramid_ms": p.value, "lk_ms": l.value, "host_ms": h.value,
                "device_bytes": m.value}


def camera_matrix(K, Rt):
    """opk_camera_matrix: the 3x4 camera matrix K [3, 3] x Rt [3, 4] (cameraParameterReader.cpp:72),
    every entry a sequential fp64 sum."""
    K = np.ascontiguousarray(K, np.float64)
    Rt = np.ascontiguousarray(Rt, np.float64)
    assert K.shape == (3, 3) and Rt.shape == (3, 4)
    out = np.zeros((3, 4), np.float64)
    check(_lib.load().opk_camera_matrix(K.ctypes.data_as(ctypes.c_void_p),
                                        Rt.ctypes.data_as(ctypes.c_void_p),
                                        out.ctypes.data_as(ctypes.c_void_p)))
    return out


KIND_3D_BODY, KIND_3D_FACE, KIND_3D_HAND_LEFT, KIND_3D_HAND_RIGHT = 0, 1, 2, 3   # OPK_3D_*


class Triangulator:
    """3-D keypoints from a camera rig (op::PoseTriangulation, --3d; include/opk.h): V = 2..7 views,
    camera_matrices [V, 3, 4] float64, image_sizes [V, 2] (width, height), min_views >= 2 or
    negative (max(2, min(4, V-1)))."""

    def __init__(self, camera_matrices, image_sizes, min_views=-1):
        self.P = np.ascontiguousarray(camera_matrices, np.float64)
        self.sizes = np.ascontiguousarray(image_sizes, np.int32)
        if self.P.ndim != 3 or self.P.shape[1:] != (3, 4) or self.sizes.shape != (self.P.shape[0], 2):
            raise ValueError("camera_matrices [V, 3, 4] and image_sizes [V, 2]")
        self.views = self.P.shape[0]
        self.min_views = int(min_views)
        # the library's checks (OPK_ERR_ARG: V outside 2..7, min_views 0 / 1, a non-finite entry)
        one = np.zeros((1, self.views, 1, 3), np.float32)
        self._host(one, np.ones((1, self.views), np.int32))

    def struct(self):
        return _lib.RigStruct(self.views, self.P.ctypes.data, self.sizes.ctypes.data, self.min_views)

    def _host(self, kp, present):
        steps, _, parts, _ = kp.shape
        xyz = np.zeros((steps, parts, 4), np.float32)
        status = np.zeros(steps, np.int32)
        errors = np.zeros((steps, parts), np.float64)
        dropped = np.zeros((steps, parts), np.int32)
        rig = self.struct()
        v = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        check(_lib.load().opk_triangulate_host(ctypes.byref(rig), steps, parts, v(kp), v(present),
                                               v(xyz), v(status), v(errors), v(dropped)))
        return xyz, status, errors, dropped

    def reconstruct(self, keypoints, present=None, device=None):
        """keypoints [steps, V, parts, 3] (x, y, score; person 0 of each view), present [steps, V]
        (default: every view has a person).  device None: opk_triangulate_host; a Context:
        opk_triangulate on its stream (numpy or CUDA inputs), bit for bit the same.  Returns (xyz
        float32 [steps, parts, 4], status int32 [steps], errors float64 [steps, parts] with -1 where
        a part was not attempted, dropped int32 [steps, parts] with -1 for none)."""
        on_dev = torch.is_tensor(keypoints)
        kshape = tuple(keypoints.shape)
        if len(kshape) != 4 or kshape[1] != self.views or kshape[3] != 3 or kshape[2] < 1:
            raise ValueError("keypoints [steps, %d, parts, 3]" % self.views)
        steps, _, parts, _ = kshape
        if present is None:
            present = np.ones((steps, self.views), np.int32)
        if device is None:
            kp = np.ascontiguousarray(keypoints.cpu().numpy() if on_dev else keypoints, np.float32)
            pr = np.ascontiguousarray(present.cpu().numpy() if torch.is_tensor(present) else present,
                                      np.int32).reshape(steps, self.views)
            return self._host(kp, pr)
        ctx = device
        kp = keypoints if on_dev else torch.from_numpy(np.ascontiguousarray(keypoints, np.float32))
        kp = kp.to("cuda", torch.float32).contiguous()
        pr = present if torch.is_tensor(present) else torch.from_numpy(
            np.ascontiguousarray(present, np.int32))
        pr = pr.to("cuda", torch.int32).reshape(steps, self.views).contiguous()
        xyz = torch.empty((steps, parts, 4), dtype=torch.float32, device="cuda")
        status = torch.empty(steps, dtype=torch.int32, device="cuda")
        errors = torch.empty((steps, parts), dtype=torch.float64, device="cuda")
        dropped = torch.empty((steps, parts), dtype=torch.int32, device="cuda")
        rig = self.struct()
        check(ctx.L.opk_triangulate(ctx.h, ctypes.byref(rig), steps, parts, _ptr(kp), _ptr(pr),
                                    _ptr(xyz), _ptr(status), _ptr(errors), _ptr(dropped)))
        ctx.sync()
        return (xyz.cpu().numpy(), status.cpu().numpy(), errors.cpu().numpy(),
                dropped.cpu().numpy())


class Cameras:
    """The lenses of a rig for the undistortion (opk_cameras, include/opk.h): intrinsics [V, 3, 3],
    distortions a list of V coefficient vectors of 4, 5, 8 or 12 values each (k1 k2 p1 p2 k3 k4 k5
    k6 s1 s2 s3 s4), image_sizes [V, 2] (width, height).  Frame f of a batch uses view f % V.  The
    reference builds every camera's map from camera 0's parameters; pass camera 0's for every view
    to reproduce that.  The library checks the values where they are used (maps,
    Context.undistort_frames, PoseExtractor.set_undistort): OPK_ERR_ARG / OPK_ERR_UNSUPPORTED."""

    def __init__(self, intrinsics, distortions, image_sizes):
        self.K = np.ascontiguousarray(intrinsics, np.float64)
        if self.K.ndim != 3 or self.K.shape[1:] != (3, 3):
            raise ValueError("intrinsics [V, 3, 3]")
        self.views = self.K.shape[0]
        dist = [np.asarray(d, np.float64).reshape(-1) for d in distortions]
        self.sizes = np.ascontiguousarray(image_sizes, np.int32)
        if len(dist) != self.views or self.sizes.shape != (self.views, 2):
            raise ValueError("one distortion vector and one (width, height) per view")
        self.ncoef = np.array([d.size for d in dist], np.int32)
        self.dist = np.zeros((self.views, 12), np.float64)
        for v, d in enumerate(dist):
            self.dist[v, :min(d.size, 12)] = d[:12]

    def struct(self):
        return _lib.CamerasStruct(self.views, self.K.ctypes.data, self.dist.ctypes.data,
                                  self.ncoef.ctypes.data, self.sizes.ctypes.data)

    def maps(self, view):
        """opk_undistort_maps_host: (m1 int16 [h, w, 2], m2 uint16 [h, w]) of one view."""
        if not 0 <= view < self.views:
            raise ValueError("bad view")
        w, h = int(self.sizes[view, 0]), int(self.sizes[view, 1])
        m1 = np.zeros((h, w, 2), np.int16)
        m2 = np.zeros((h, w), np.uint16)
        s = self.struct()
        check(_lib.load().opk_undistort_maps_host(ctypes.byref(s), view,
                                                  m1.ctypes.data_as(ctypes.c_void_p),
                                                  m2.ctypes.data_as(ctypes.c_void_p)))
        return m1, m2


class CameraParameters:
    """The calibration files of a rig (op::CameraParameterReader::readParameters): one
    <dir>/<serial>.xml per camera.  serials: the cameras in rig order, one of them .intrinsics
    [V, 3, 3], .distortions (a list of V vectors), .extrinsics [V, 3, 4] (the files' CameraMatrix),
    .extrinsics_initial [V, 3, 4] (CameraMatrixInitial, the identity where a file has none) and
    .camera_matrices [V, 3, 4] = intrinsics x extrinsics."""

    def __init__(self, serials, intrinsics, distortions, extrinsics, extrinsics_initial,
                 camera_matrices):
        self.serials, self.intrinsics, self.distortions = serials, intrinsics, distortions
        self.extrinsics, self.extrinsics_initial = extrinsics, extrinsics_initial
        self.camera_matrices = camera_matrices

    @classmethod
    def read(cls, directory, serials=None):
        """opk_camera_parameters_read; serials None: every *.xml of the directory, sorted."""
        L = _lib.load()
        d = os.fsencode(str(directory))
        count = ctypes.c_int(0)
        if serials is None:
            names, n = None, 0
            check(L.opk_camera_parameters_read(d, None, 0, None, 0, ctypes.byref(count)))
        else:
            n = len(serials)
            names = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(str(x)) for x in serials])
            count.value = n
        out = (_lib.CameraParametersStruct * max(count.value, 1))()
        check(L.opk_camera_parameters_read(d, names, n, ctypes.byref(out), count.value,
                                           ctypes.byref(count)))
        cams = [out[i] for i in range(count.value)]
        arr = lambda field, shape: np.array([list(getattr(c, field)) for c in cams],
                                            np.float64).reshape((len(cams),) + shape)
        return cls([os.fsdecode(c.serial) for c in cams], arr("intrinsics", (3, 3)),
                   [np.array(list(c.distortion)[:c.ncoef], np.float64) for c in cams],
                   arr("extrinsics", (3, 4)), arr("extrinsics_initial", (3, 4)),
                   arr("camera_matrix", (3, 4)))

    def _sizes(self, image_sizes):
        sizes = np.asarray(image_sizes, np.int32)
        if sizes.shape == (2,):
            sizes = np.tile(sizes, (len(self.serials), 1))
        return sizes

    def triangulator(self, image_sizes, min_views=-1):
        """The Triangulator of these cameras; image_sizes [V, 2] or one (width, height) for all."""
        return Triangulator(self.camera_matrices, self._sizes(image_sizes), min_views)

    def cameras(self, image_sizes):
        """The Cameras (undistortion) of these cameras, each view with its own parameters."""
        return Cameras(self.intrinsics, self.distortions, self._sizes(image_sizes))


class _DeviceBytes:
    """Library-owned device memory as a uint8 tensor (torch.as_tensor reads this interface)."""

    def __init__(self, ptr, shape, strides):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "|u1", "data": (ptr, False),
                                         "version": 2, "strides": strides}


class Net:
    """op::NetCaffe replacement (NetHip): prototxt path or "builtin:BODY_25"."""

    def __init__(self, ctx, prototxt="builtin:BODY_25", caffemodel=None):
        self.ctx = ctx
        self.L = ctx.L
        h = ctypes.c_void_p()
        check(self.L.opk_net_create(ctx.h, prototxt.encode(),
                                    caffemodel.encode() if caffemodel else None, ctypes.byref(h)))
        self.h = h
        _LIVE["net"].add(self)

    def close(self):
        if self.h:
            self.L.opk_net_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def convs(self):
        """[{name, cin, num_output, kernel_size, act}] in execution order."""
        out = []
        name = ctypes.create_string_buffer(64)
        cin, cout, k, act = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        for i in range(self.L.opk_net_num_convs(self.h)):
            check(self.L.opk_net_conv_info(self.h, i, name, ctypes.byref(cin), ctypes.byref(cout),
                                           ctypes.byref(k), ctypes.byref(act)))
            out.append(dict(name=name.value.decode(), cin=cin.value, num_output=cout.value,
                            kernel_size=k.value, act=act.value))
        return out

    def set_params(self, params):
        """params: {conv name: (w [co,ci,k,k], bias [co], slope [co] | None)} fp32 numpy."""
        for c in self.convs():
            w, b, s = params[c["name"]]
            w = np.ascontiguousarray(w, np.float32)
            b = np.ascontiguousarray(b, np.float32)
            sp = None
            if s is not None:
                s = np.ascontiguousarray(s, np.float32)
                sp = s.ctypes.data_as(ctypes.c_void_p)
            check(self.L.opk_net_set_conv(self.h, c["name"].encode(),
                                          w.ctypes.data_as(ctypes.c_void_p),
                                          b.ctypes.data_as(ctypes.c_void_p), sp))

    def forward(self, x):
        """x: [n, 3, h, w] fp32 CUDA tensor. Returns (device pointer, shape) of net_output."""
        n, c, h, w = x.shape
        check(self.L.opk_net_forward(self.h, _ptr(x), n, h, w))
        return self.output()

    def load_caffemodel(self, path):
        """Trained weights (CopyTrainedLayersFrom semantics); returns the convs loaded."""
        n = ctypes.c_int()
        check(self.L.opk_net_load_caffemodel(self.h, path.encode(), ctypes.byref(n)))
        return n.value

    def set_precision(self, precision):
        """PRECISION_FP16 (default) or PRECISION_SPLIT (fp16 hi/lo pairs, ~fp32 results at ~3x
        the MFMA work; opk_net_set_precision)."""
        check(self.L.opk_net_set_precision(self.h, int(precision)))

    def set_precision_schedule(self, schedule):
        """Per-layer precision (opk_net_set_precision_schedule).  schedule: a sequence of one
        PRECISION_FP16 / PRECISION_SPLIT per conv in convs() order; a {conv name: precision} dict
        (convs it does not name keep theirs); or a callable taking a convs() entry (plus its
        "index") and returning the precision.  Refused schedules leave the one in force."""
        convs = self.convs()
        if callable(schedule):
            sched = [schedule(dict(c, index=i)) for i, c in enumerate(convs)]
        elif isinstance(schedule, dict):
            names = {c["name"] for c in convs}
            unknown = sorted(set(schedule) - names)
            if unknown:
                raise OpkError("precision schedule: no convolution named " + ", ".join(unknown))
            cur = self.precision_schedule()
            sched = [schedule.get(c["name"], cur[i]) for i, c in enumerate(convs)]
        else:
            sched = list(schedule)
        arr = (ctypes.c_int * max(1, len(sched)))(*[int(p) for p in sched])
        check(self.L.opk_net_set_precision_schedule(self.h, arr, len(sched)))

    def precision_schedule(self):
        """The precision of every conv, in convs() order."""
        return [self.L.opk_net_conv_precision(self.h, i)
                for i in range(self.L.opk_net_num_convs(self.h))]

    def set_small_batch(self, on=True):
        """Small-batch mode (opk_net_set_small_batch): 3x3 layers that would not fill the chip run
        on conv3s tiles; the results are bit-identical."""
        check(self.L.opk_net_set_small_batch(self.h, int(bool(on))))

    @property
    def small_batch(self):
        return self.L.opk_net_small_batch(self.h) == 1

    def conv_plan(self, index, n, h, w, cus):
        """{bm, bn, workgroups, small} the planner picks for conv `index` (convs() order) of an
        n x h x w forward on a chip of `cus` compute units (opk_net_conv_plan; host-only)."""
        v = [ctypes.c_int() for _ in range(4)]
        check(self.L.opk_net_conv_plan(self.h, index, n, h, w, cus, *[ctypes.byref(x) for x in v]))
        return dict(bm=v[0].value, bn=v[1].value, workgroups=v[2].value, small=v[3].value)

    def conv_kernels(self, index, n, h, w, cus):
        """Launch-log name prefixes of the launches such a forward makes for conv `index`, in
        launch order (opk_net_conv_kernels; host-only): one per frame run, none for a conv inside
        another conv's fused kernel."""
        need = ctypes.c_size_t()
        check(self.L.opk_net_conv_kernels(self.h, index, n, h, w, cus, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        check(self.L.opk_net_conv_kernels(self.h, index, n, h, w, cus, buf, need.value, ctypes.byref(need)))
        return buf.value.decode().splitlines()

    def set_timing(self, on=True):
        check(self.L.opk_net_set_timing(self.h, int(on)))

    def read_timing(self):
        """(forwards, summed device ms) since the last read (HIP events on the context stream)."""
        n, ms = ctypes.c_int(), ctypes.c_double()
        check(self.L.opk_net_read_timing(self.h, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    def flops_per_frame(self, h, w):
        f = ctypes.c_double()
        check(self.L.opk_net_flops_per_frame(self.h, h, w, ctypes.byref(f)))
        return f.value

    def output(self):
        p = ctypes.c_void_p()
        shape = (ctypes.c_int * 4)()
        check(self.L.opk_net_output(self.h, ctypes.byref(p), shape))
        return p.value, tuple(shape)

    def output_numpy(self):
        p, shape = self.output()
        out = np.empty(shape, np.float32)
        check(self.L.opk_memcpy_d2h(self.ctx.h, out.ctypes.data_as(ctypes.c_void_p),
                                    ctypes.c_void_p(p), out.nbytes))
        return out

    def blob(self, name, frames=None):
        """Named top of the last forward (opk_net_blob) as fp32 NCHW numpy: frames = (first, count),
        default all.  Values are the fp16 activations the kernels stored (net_output: fp32)."""
        shape = (ctypes.c_int * 4)()
        f0, nf = frames if frames is not None else (0, self.output()[1][0])
        check(self.L.opk_net_blob(self.h, name.encode(), f0, nf, None, shape))
        out = np.empty(tuple(shape), np.float32)
        check(self.L.opk_net_blob(self.h, name.encode(), f0, nf,
                                  out.ctypes.data_as(ctypes.c_void_p), shape))
        return out

    def blob_planes(self, name, frames=None):
        """(hi, lo, has_lo) of a named top of the last forward (opk_net_blob_planes): the stored hi
        image and its lo twin as fp32 NCHW numpy; a buffer without a twin gives zeros and False."""
        shape = (ctypes.c_int * 4)()
        has = ctypes.c_int()
        f0, nf = frames if frames is not None else (0, self.output()[1][0])
        check(self.L.opk_net_blob_planes(self.h, name.encode(), f0, nf, None, None, shape,
                                         ctypes.byref(has)))
        hi = np.empty(tuple(shape), np.float32)
        lo = np.empty(tuple(shape), np.float32)
        check(self.L.opk_net_blob_planes(self.h, name.encode(), f0, nf,
                                         hi.ctypes.data_as(ctypes.c_void_p),
                                         lo.ctypes.data_as(ctypes.c_void_p), shape, ctypes.byref(has)))
        return hi, lo, bool(has.value)

    def launch_log(self):
        """[(layer, kernel instantiation)] of the last forward run under dev_switches(LAUNCH_LOG=1)."""
        need = ctypes.c_size_t()
        check(self.L.opk_net_launch_log(self.h, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        check(self.L.opk_net_launch_log(self.h, buf, need.value, ctypes.byref(need)))
        return [tuple(line.split("\t", 1)) for line in buf.value.decode().splitlines()]


class PoseExtractor:
    """op::PoseExtractorCaffe replacement for batches of frames (PoseHip)."""

    def __init__(self, ctx, net=None, maximize_positives=False, pose_model=BODY_25,
                 semantics=CONNECT_CPU):
        self.ctx = ctx
        self.L = ctx.L
        h = ctypes.c_void_p()
        check(self.L.opk_pose_create_model(ctx.h, net.h if net is not None else None, pose_model,
                                           int(maximize_positives), semantics, ctypes.byref(h)))
        self.h = h
        _LIVE["pose"].add(self)
        self.net = net
        self.parts = pose_model_info(pose_model)["parts"]
        self.pose_model = pose_model
        self._attached = {}   # kind -> KeypointExtractor (kept alive while attached)
        self._tracker = None  # the attached Tracker
        self._views = None    # the Triangulator of set_views
        self._undistort = None   # the Cameras of set_undistort

    def close(self):
        if self.h:
            self.L.opk_pose_destroy(self.h)
            self.h = None
            self._attached = {}
            self._tracker = None
            self._views = None

    # ---- face / hand stages (opk_pose_attach_extractor) ---------------------------------------
    def attach(self, face=None, hands=None, tracker=None):
        """Run these KeypointExtractors (kind FACE / HAND) inside collect(): rectangles from each
        frame's pose keypoints, then the extractor on the batch's frames.  Only forward_frames /
        submit_frames are accepted while one is attached, and a submitted batch's frames must stay
        unchanged until it is collected.
        tracker: a Tracker under the same rules (opk_pose_attach_tracker): the batch's pyramid is
        queued at submit, collect() runs its update on the batch's keypoints -- person_ids(frame)."""
        if tracker is not None:
            check(self.L.opk_pose_attach_tracker(self.h, tracker.h))
            self._tracker = tracker
        for ex, kind in ((face, FACE), (hands, HAND)):
            if ex is None:
                continue
            if ex.kind != kind:
                raise ValueError("face wants a FACE extractor, hands a HAND extractor")
            check(self.L.opk_pose_attach_extractor(self.h, ex.h))
            self._attached[kind] = ex

    def detach(self, kind):
        check(self.L.opk_pose_detach_extractor(self.h, kind))
        self._attached.pop(kind, None)

    def detach_tracker(self):
        check(self.L.opk_pose_detach_tracker(self.h))
        self._tracker = None

    # ---- 3-D keypoints (opk_pose_set_views) ----------------------------------------------------
    def set_views(self, tri):
        """A Triangulator: from now on a batch of n frames is n / V time steps of its rig, frame
        t*V + v the view v of step t, and collect() reconstructs person 0 of every step --
        keypoints_3d(step), datum(frame).  None clears.  Not with batches in flight.
        The mode is the reference's --3d, which demands --number_people_max 1: only person 0 of a
        frame is reconstructed, and people_json refuses a datum whose 2-D arrays hold more people
        than its 3-D ones -- cut such a frame to its first person before writing it."""
        if tri is None:
            check(self.L.opk_pose_set_views(self.h, None))
        else:
            rig = tri.struct()
            check(self.L.opk_pose_set_views(self.h, ctypes.byref(rig)))
        self._views = tri

    def keypoints_3d(self, step):
        """The four 3-D arrays of a collected time step, body, face, left hand, right hand: each
        float32 [1, parts, 4] (x, y, z, 1 or zeros), or empty where the step's status is 0 or the
        extractor is not attached."""
        out = []
        for kind, on, parts in ((KIND_3D_BODY, True, self.parts),
                                (KIND_3D_FACE, FACE in self._attached, 70),
                                (KIND_3D_HAND_LEFT, HAND in self._attached, 21),
                                (KIND_3D_HAND_RIGHT, HAND in self._attached, 21)):
            if kind and on:
                parts = self._attached[FACE if kind == KIND_3D_FACE else HAND].parts
            xyz = np.zeros((1, parts, 4), np.float32)
            st = ctypes.c_int(0)
            if on or not kind:
                check(self.L.opk_pose_keypoints_3d(self.h, step, kind,
                                                   xyz.ctypes.data_as(ctypes.c_void_p),
                                                   ctypes.byref(st)))
            out.append(xyz if st.value else np.zeros((0, parts, 4), np.float32))
        return out

    # ---- undistortion (opk_pose_set_undistort) -------------------------------------------------
    def set_undistort(self, cameras):
        """A Cameras: from now on submit_frames / forward_frames first undistort the batch (frame f
        through view f % V) into a BGR buffer of the batch's slot, and every later stage -- the
        warp, the tracker, the face / hand crops -- reads that; undistorted_frames() hands it out
        for the renders.  None clears and frees the slots' buffers.  Not with batches in flight.
        130 frames of 1280x720 are 360 MB per slot, two slots; the context keeps the maps of every
        distinct camera set it has seen (5.5 MB per camera at 1280x720) until it is closed."""
        if cameras is None:
            check(self.L.opk_pose_set_undistort(self.h, None))
        else:
            c = cameras.struct()
            check(self.L.opk_pose_set_undistort(self.h, ctypes.byref(c)))
        self._undistort = cameras

    def undistorted_frames(self):
        """The collected batch's undistorted frames as a BGR Frames over the pipeline's buffer (no
        copy): valid until the second submit after that batch's or set_undistort(None)."""
        f = _lib.FramesStruct()
        check(self.L.opk_pose_undistorted_frames(self.h, ctypes.byref(f)))
        step, frame = int(f.step[0]), int(f.frame_bytes[0])
        t = torch.as_tensor(_DeviceBytes(int(f.plane[0]), (f.n, f.height, f.width * 3),
                                         (frame, step, 1)), device="cuda")
        return Frames.bgr(t, f.width)

    # ---- orientation (opk_pose_set_orientation) ------------------------------------------------
    def set_orientation(self, rotate=0, flip=False):
        """--frame_rotate / --frame_flip: from now on submit_frames / forward_frames rotate and
        mirror the batch (after the undistortion, if set) into a buffer of the batch's slot, in the
        frames' own format, and every later stage reads that: keypoints come out in the oriented
        frame's coordinates (orient_keypoints(..., inverse=True) takes them back), and a rig set
        with set_views must be one of the oriented images.  (0, False) clears and frees the slots'
        buffers.  Not with batches in flight."""
        check(self.L.opk_pose_set_orientation(self.h, int(rotate), int(flip)))

    def oriented_frames(self):
        """The collected batch's oriented frames as a Frames over the pipeline's buffer (no copy):
        valid until the second submit after that batch's or set_orientation(0, False)."""
        f = _lib.FramesStruct()
        check(self.L.opk_pose_oriented_frames(self.h, ctypes.byref(f)))

        def plane(i, rows, row_bytes):
            return torch.as_tensor(_DeviceBytes(int(f.plane[i]), (f.n, rows, row_bytes),
                                                (int(f.frame_bytes[i]), int(f.step[i]), 1)),
                                   device="cuda")
        w, h = f.width, f.height
        if f.format == FRAMES_BGR:
            return Frames.bgr(plane(0, h, w * 3), w)
        if f.format == FRAMES_NV12:
            return Frames.nv12(plane(0, h, w), plane(1, h // 2, w), w)
        return Frames.i420(plane(0, h, w), plane(1, h // 2, w // 2), plane(2, h // 2, w // 2), w)

    def person_ids(self, frame):
        """int64 [people] ids of a collected frame, person order of keypoints() (needs a tracker)."""
        ids = np.full(max(self.num_people(frame), 0), -2, np.int64)
        check(self.L.opk_pose_person_ids(self.h, frame, ids.ctypes.data_as(ctypes.c_void_p)))
        return ids

    def read_track_times(self):
        """{batches, pyramid_ms, lk_ms, host_ms} of the attached tracker since the last read."""
        b, p, l, h = ctypes.c_int(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        check(self.L.opk_pose_read_track_times(self.h, ctypes.byref(b), ctypes.byref(p),
                                               ctypes.byref(l), ctypes.byref(h)))
        return {"batches": b.value, "pyramid_ms": p.value, "lk_ms": l.value, "host_ms": h.value}

    def _part_rectangles(self, kind, frame):
        n = max(self.num_people(frame), 0)
        out = np.zeros((n, 2 if kind == HAND else 1, 4), np.float32)
        check(self.L.opk_pose_part_rectangles(self.h, kind, frame,
                                              out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def _part_keypoints(self, kind, frame):
        n = max(self.num_people(frame), 0)
        parts = self._attached[kind].parts if kind in self._attached else (21 if kind == HAND else 70)
        out = np.zeros((2 if kind == HAND else 1, n, parts, 3), np.float32)
        check(self.L.opk_pose_part_keypoints(self.h, kind, frame,
                                             out.ctypes.data_as(ctypes.c_void_p), n))
        return out

    def face_rectangles(self, frame):
        """[people, 4] (x, y, width, height) of a collected frame, person order of keypoints()."""
        return self._part_rectangles(FACE, frame)[:, 0]

    def hand_rectangles(self, frame):
        """[people, 2 (left, right), 4]."""
        return self._part_rectangles(HAND, frame)

    def face_keypoints(self, frame):
        """[people, 70, 3]; zeros where the reference skips the rectangle."""
        return self._part_keypoints(FACE, frame)[0]

    def hand_keypoints(self, frame):
        """[2 (left, right), people, 21, 3]."""
        return self._part_keypoints(HAND, frame)

    def datum(self, frame):
        """datum_keypoint_vector of a collected frame: pose and, for the attached extractors, face
        and both hands -- ready for people_json / save_people_json.  With a tracker attached
        "person_id" holds its ids, else -1 each.  With views set (set_views) the four 3-D arrays of
        the frame's time step come with it; they hold person 0 only, so for people_json the frame
        must hold one person (--number_people_max 1) or be cut to its first."""
        face = self.face_keypoints(frame) if FACE in self._attached else None
        hands = tuple(self.hand_keypoints(frame)) if HAND in self._attached else (None, None)
        ids = self.person_ids(frame) if self._tracker is not None else None
        if self._views is None:
            return datum_keypoint_vector(self.keypoints(frame)[0], face, hands, ids)
        # every frame of a time step carries the step's 3-D arrays (wPoseTriangulation.hpp:94-100)
        body3, face3, left3, right3 = self.keypoints_3d(frame // self._views.views)
        return datum_keypoint_vector(self.keypoints(frame)[0], face, hands, ids, body3, face3,
                                     (left3, right3))

    def read_part_times(self, kind):
        """{batches, crops, host_ms, wait_ms} of the stage since the last read: host time for
        rectangles, crop validity and tables; time waiting for the device."""
        b, c = ctypes.c_int(0), ctypes.c_int(0)
        h, w = ctypes.c_double(0), ctypes.c_double(0)
        check(self.L.opk_pose_read_part_times(self.h, kind, ctypes.byref(b), ctypes.byref(c),
                                              ctypes.byref(h), ctypes.byref(w)))
        return {"batches": b.value, "crops": c.value, "host_ms": h.value, "wait_ms": w.value}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_property(self, prop, value):
        check(self.L.opk_pose_set_property(self.h, prop, float(value)))

    def set_map_semantics(self, semantics):
        """MAPS_CPU (default) or MAPS_CUDA: the resize + NMS arithmetic of the reference's CPU or
        CUDA build (opk_pose_set_map_semantics)."""
        check(self.L.opk_pose_set_map_semantics(self.h, semantics))

    def set_upsampling_ratio(self, ratio):
        """--upsampling_ratio (PoseExtractorCaffe's upsamplingRatio): heat maps at
        round(out * ratio - 1) + 1 instead of the net input size; <= 0 restores the default."""
        check(self.L.opk_pose_set_upsampling_ratio(self.h, float(ratio)))

    def set_overlay(self, overlay):
        self._overlay = overlay   # keep the tensor alive
        check(self.L.opk_pose_set_overlay(self.h, _ptr(overlay) if overlay is not None else None))

    def forward(self, frames, producer_size):
        n, _, h, w = frames.shape
        check(self.L.opk_pose_forward(self.h, _ptr(frames), n, h, w, producer_size[0],
                                      producer_size[1]))

    def _multi(self, fn, frames, producer_size):
        n = frames[0].shape[0]
        ptrs = (ctypes.c_void_p * len(frames))(*[f.data_ptr() for f in frames])
        for f in frames:
            assert f.is_cuda and f.is_contiguous() and f.shape[0] == n
        hw = (ctypes.c_int * (2 * len(frames)))(*[v for f in frames for v in f.shape[2:]])
        check(fn(self.h, ptrs, hw, len(frames), n, producer_size[0], producer_size[1]))

    def forward_multi(self, frames, producer_size):
        """Multi-scale: frames = list of [n,3,h_i,w_i] net inputs, scale 0 first."""
        self._multi(self.L.opk_pose_forward_multi, frames, producer_size)

    def submit_multi(self, frames, producer_size):
        self._multi(self.L.opk_pose_submit_multi, frames, producer_size)

    def set_input(self, net_resolution=(-1, 368), dynamic_behavior=1.0, scale_number=1,
                  scale_gap=0.25):
        """--net_resolution, --net_resolution_dynamic, --scale_number, --scale_gap."""
        check(self.L.opk_pose_set_input(self.h, net_resolution[0], net_resolution[1],
                                        float(dynamic_behavior), scale_number, float(scale_gap)))

    def _frames(self, fn, frames):
        frames = _as_frames(frames)
        s = frames.struct()
        check(fn(self.h, ctypes.byref(s)))
        self._frames_n = frames.n

    def forward_frames(self, frames):
        """Raw BGR uint8 frames [n, h, w, 3] (CUDA), or a Frames (BGR, NV12, I420): GPU
        preprocessing + net + post-processing."""
        self._frames(self.L.opk_pose_forward_frames_fmt, frames)

    def submit_frames(self, frames):
        self._frames(self.L.opk_pose_submit_frames_fmt, frames)

    def net_input_numpy(self, scale=0):
        p = ctypes.c_void_p()
        w, h = ctypes.c_int(), ctypes.c_int()
        check(self.L.opk_pose_net_input(self.h, scale, ctypes.byref(p), ctypes.byref(w),
                                        ctypes.byref(h)))
        n = self._frames_n
        out = np.empty((n, 3, h.value, w.value), np.float32)
        check(self.L.opk_memcpy_d2h(self.ctx.h, out.ctypes.data_as(ctypes.c_void_p), p, out.nbytes))
        return out

    def forward_net_output(self, net_output, net_size, producer_size):
        """net_output: [n, heat_channels, h, w] CUDA tensor (or (ptr, shape)); net_size = (w, h)."""
        if isinstance(net_output, tuple):
            ptr, shape = net_output
            ptr = ctypes.c_void_p(ptr)
        else:
            ptr, shape = _ptr(net_output), net_output.shape
        check(self.L.opk_pose_forward_net_output(self.h, ptr, shape[0], shape[2], shape[3],
                                                 net_size[1], net_size[0], producer_size[0],
                                                 producer_size[1]))

    def submit(self, frames, producer_size):
        """Enqueue a batch's device work and return (pipelined use; see opk_pose_submit)."""
        n, _, h, w = frames.shape
        check(self.L.opk_pose_submit(self.h, _ptr(frames), n, h, w, producer_size[0],
                                     producer_size[1]))

    def submit_net_output(self, net_output, net_size, producer_size):
        if isinstance(net_output, tuple):
            ptr, shape = net_output
            ptr = ctypes.c_void_p(ptr)
        else:
            ptr, shape = _ptr(net_output), net_output.shape
        check(self.L.opk_pose_submit_net_output(self.h, ptr, shape[0], shape[2], shape[3],
                                                net_size[1], net_size[0], producer_size[0],
                                                producer_size[1]))

    def collect(self):
        """Wait for the oldest submitted batch, assemble its people; returns its frame count."""
        n = ctypes.c_int(0)
        check(self.L.opk_pose_collect(self.h, ctypes.byref(n)))
        return n.value

    def pending(self):
        return self.L.opk_pose_pending(self.h)

    def num_people(self, frame):
        return self.L.opk_pose_num_people(self.h, frame)

    def keypoints(self, frame):
        n = self.num_people(frame)
        kp = np.zeros((max(n, 1), self.parts, 3), np.float32)
        ks = np.zeros(max(n, 1), np.float32)
        check(self.L.opk_pose_keypoints(self.h, frame, kp.ctypes.data_as(ctypes.c_void_p),
                                        ks.ctypes.data_as(ctypes.c_void_p), n))
        return kp[:n], ks[:n]

    def render_frames(self, frames, scale=1.0, out_size=None, threshold=0.05, alpha=0.6,
                      googly_eyes=False, blend_original=True, cast=CAST_CPU, out=None, element=0,
                      alpha_heatmap=0.7, face=False, hands=False, face_threshold=0.4,
                      face_alpha=0.6, hand_threshold=0.2, hand_alpha=0.6, out_format=None):
        """The last collected batch drawn on its frames [n, h, w, 3] uint8 BGR (CUDA) ->
        uint8 [n, out_h, out_w, 3]; keypoints are scaled by `scale` (scaleInputToOutput).
        element (--part_to_show, see render_element): 0 the keypoints; any other draws that heat
        map / PAF of the batch instead, evaluated from the net output (no full-resolution stack
        is written), blended with alpha_heatmap.
        face / hands: also draw the attached extractors' results (attach) as a FACE and a HAND
        layer after the POSE layer (opk_pose_render_frames_parts_fmt when the flags name every attached
        extractor; a subset is put together from the accessors and drawn by Context.render_frames,
        the same bytes).  frames may be a Frames (BGR, NV12 or I420).
        Frames out: a Frames as `out` (BGR, NV12 or I420), or out_format="nv12" | "i420", takes
        the drawn frames (opk_pose_render_frames_to) and is returned, as Context.render_frames."""
        frames = _as_frames(frames)
        fs, n = frames.struct(), frames.n
        ow, oh = out_size if out_size is not None else (frames.width, frames.height)
        dest = _frames_out(out, out_format, n, oh, ow, frames.device)
        if dest is not None:
            out = dest
        elif out is None:
            out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=frames.device)
        every = False
        if face or hands:
            if element != 0:
                raise ValueError("face / hand layers are drawn with the keypoints (element 0)")
            if (face and FACE not in self._attached) or (hands and HAND not in self._attached):
                raise ValueError("no such extractor attached")
            every = bool(face) == (FACE in self._attached) and bool(hands) == (HAND in self._attached)
        if dest is not None and (every or not (face or hands)):
            ds = dest.struct_out()
            parts = None
            if every:
                parts = (ctypes.c_float * 4)(face_threshold, face_alpha, hand_threshold, hand_alpha)
            check(self.L.opk_pose_render_frames_to(
                self.h, ctypes.byref(ds), ctypes.byref(fs), float(scale), int(element), threshold,
                alpha, alpha_heatmap, int(googly_eyes), int(blend_original), cast, parts))
            return dest
        if face or hands:
            if every:   # every attached extractor's layer
                check(self.L.opk_pose_render_frames_parts_fmt(
                    self.h, _ptr(out), _row_bytes(out, n, oh, ow), ow, oh, ctypes.byref(fs),
                    float(scale), threshold, alpha, int(googly_eyes), int(blend_original), cast,
                    face_threshold, face_alpha, hand_threshold, hand_alpha))
                return out
            # a subset of the attached extractors: the same layers, put together here
            s = np.float32(scale)

            def layer(kind, arrays, per, th, al, **kw):
                kp = np.concatenate(arrays).astype(np.float32)
                kp[..., :2] *= s   # scaleKeypoints: x and y times scaleInputToOutput, in float
                dev = torch.from_numpy(np.ascontiguousarray(kp)).to(frames.device) if kp.size else None
                return RenderLayer(kind, dev, [per * c for c in counts], th, al, **kw)

            counts = [self.num_people(f) for f in range(n)]
            layers = [layer(LAYER_POSE, [self.keypoints(f)[0] for f in range(n)], 1, threshold,
                            alpha, pose_model=self.pose_model, googly_eyes=googly_eyes)]
            if face:
                layers.append(layer(LAYER_FACE, [self.face_keypoints(f) for f in range(n)], 1,
                                    face_threshold, face_alpha))
            if hands:   # a frame's left hands, then its right hands
                parts = self._attached[HAND].parts
                layers.append(layer(LAYER_HAND, [self.hand_keypoints(f).reshape(-1, parts, 3)
                                                 for f in range(n)], 2, hand_threshold, hand_alpha))
            return self.ctx.render_frames(frames, layers, scale, out_size, blend_original, cast, out)
        check(self.L.opk_pose_render_frames_element_fmt(
            self.h, _ptr(out), _row_bytes(out, n, oh, ow), ow, oh, ctypes.byref(fs), float(scale),
            int(element), threshold, alpha, alpha_heatmap, int(googly_eyes), int(blend_original),
            cast))
        return out

    def write_images(self, directory, names, frames, quality=100, **render_args):
        """--write_images <directory> --write_images_format jpg: the last collected batch drawn on
        `frames` (render_frames with render_args, into a BGR buffer this object keeps), encoded
        (Context.encode_jpeg) and saved as <name>_rendered.jpg (JpegBatch.save).  frames as for
        render_frames, undistorted_frames() and oriented_frames() included.  Returns the paths."""
        if "out" in render_args or "out_format" in render_args:
            raise ValueError("write_images draws into its own BGR buffer")
        src = _as_frames(frames)
        ow, oh = render_args.get("out_size") or (src.width, src.height)
        buf = getattr(self, "_write_bgr", None)
        if buf is None or buf.numel() < src.n * oh * ow * 3 or buf.device != src.device:
            buf = self._write_bgr = torch.empty(src.n * oh * ow * 3, dtype=torch.uint8,
                                                device=src.device)
        drawn = buf[:src.n * oh * ow * 3].view(src.n, oh, ow, 3)
        self.render_frames(src, out=drawn, **render_args)
        return self.ctx.encode_jpeg(drawn, quality).save(directory, names)

    def set_timing(self, on=True):
        check(self.L.opk_pose_set_timing(self.h, int(on)))

    def read_timing(self):
        """(batches, summed post-processing device ms) since the last read."""
        n, ms = ctypes.c_int(0), ctypes.c_double(0)
        check(self.L.opk_pose_read_timing(self.h, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    def read_collect_times(self):
        """{collects, wait_ms, assembly_ms, workers} of the collects since the last read (host
        time waiting for the device results vs assembling people; opk_pose_read_collect_times)."""
        n, w, a, k = ctypes.c_int(0), ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
        check(self.L.opk_pose_read_collect_times(self.h, ctypes.byref(n), ctypes.byref(w),
                                                 ctypes.byref(a), ctypes.byref(k)))
        return {"collects": n.value, "wait_ms": w.value, "assembly_ms": a.value, "workers": k.value}

    def records(self, out=None):
        """Packed results of every frame of the last collected batch (opk_pose_records):
        per frame [people, keypoints (people x parts x 3), scores (people)], float32.  With `out`
        (a float32 numpy buffer) the records are written there; returns the filled view."""
        used = ctypes.c_size_t(0)
        check(self.L.opk_pose_records(self.h, None, 0, ctypes.byref(used)))
        if out is None:
            out = np.empty(used.value, np.float32)
        if out.size < used.value:
            raise ValueError("records buffer holds %d floats, %d needed" % (out.size, used.value))
        check(self.L.opk_pose_records(self.h, out.ctypes.data_as(ctypes.c_void_p), out.size,
                                      ctypes.byref(used)))
        return out[:used.value]

    def scale_net_to_output(self):
        return self.L.opk_pose_scale_net_to_output(self.h)

    def _dev_array(self, fn):
        p = ctypes.c_void_p()
        shape = (ctypes.c_int * 4)()
        check(fn(self.h, ctypes.byref(p), shape))
        out = np.empty(tuple(shape), np.float32)
        check(self.L.opk_memcpy_d2h(self.ctx.h, out.ctypes.data_as(ctypes.c_void_p), p, out.nbytes))
        return out

    def heatmaps_numpy(self):
        return self._dev_array(self.L.opk_pose_heatmaps)

    def heatmaps_copy(self, types=7, scale_mode=8):
        """getHeatMapsCopy for every frame of the last batch: [n, channels, H, W] float32 numpy
        (types bits: 1 parts, 2 background, 4 PAFs; scale_mode: op::ScaleMode value)."""
        shape = (ctypes.c_int * 4)()
        check(self.L.opk_pose_heatmaps_copy(self.h, types, scale_mode, None, shape))
        dev = torch.empty(tuple(shape), dtype=torch.float32, device="cuda")
        check(self.L.opk_pose_heatmaps_copy(self.h, types, scale_mode, _ptr(dev), shape))
        return dev.cpu().numpy()

    def heatmaps_copy_range(self, types=7, scale_mode=8, frames=None, dtype=torch.float32, out=None):
        """heatmaps_copy's values for frames = (first, count) of the last batch (None: all), as a
        CUDA tensor [count, channels, H, W], written straight from the net output: the
        full-resolution stack is never materialised (opk_pose_heatmaps_copy_range).  dtype
        torch.float32, or torch.uint8 with scale_mode 7 (UnsignedChar): min(value, 255)."""
        if dtype not in (torch.float32, torch.uint8):
            raise ValueError("heat maps are float32 or uint8")
        f0, nf = (0, -1) if frames is None else (int(frames[0]), int(frames[1]))
        kind = 0 if dtype == torch.float32 else 2   # OPK_F32 / OPK_U8
        shape = (ctypes.c_int * 4)()
        check(self.L.opk_pose_heatmaps_copy_range(self.h, types, scale_mode, f0, nf, None, kind,
                                                  shape))
        if out is None:
            out = torch.empty(tuple(shape), dtype=dtype, device="cuda")
        assert out.dtype == dtype and tuple(out.shape) == tuple(shape) and out.is_contiguous()
        check(self.L.opk_pose_heatmaps_copy_range(self.h, types, scale_mode, f0, nf, _ptr(out),
                                                  kind, shape))
        return out

    def candidates(self, frame):
        """getCandidatesCopy: list over parts of [count, 3] arrays (x, y output pixels, score)."""
        out = np.zeros((self.parts, 127, 3), np.float32)
        counts = np.zeros(self.parts, np.int32)
        check(self.L.opk_pose_candidates(self.h, frame, out.ctypes.data_as(ctypes.c_void_p),
                                         counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
        return [out[p, :counts[p]].copy() for p in range(self.parts)]

    def peaks_numpy(self):
        return self._dev_array(self.L.opk_pose_peaks)


# ---- face / hand keypoints ---------------------------------------------------------------------
FACE, HAND = 0, 1


def _detect(fn, pose_model, keypoints, per_person):
    kp = np.ascontiguousarray(keypoints, np.float32)
    people, parts = kp.shape[0], (kp.shape[1] if kp.ndim == 3 else 0)
    out = np.zeros((people, per_person, 4), np.float32)
    check(fn(pose_model, kp.ctypes.data_as(ctypes.c_void_p), people, parts,
             out.ctypes.data_as(ctypes.c_void_p)))
    return out


def detect_faces(pose_keypoints, pose_model=BODY_25):
    """op::FaceDetector(poseModel).detectFaces: [people, 4] (x, y, width, height)."""
    return _detect(_lib.load().opk_face_detect, pose_model, pose_keypoints, 1)[:, 0]


def detect_hands(pose_keypoints, pose_model=BODY_25):
    """op::HandDetector(poseModel).detectHands: [people, 2 (left, right), 4]."""
    return _detect(_lib.load().opk_hand_detect, pose_model, pose_keypoints, 2)


class KeypointExtractor:
    """op::FaceExtractorCaffe / op::HandExtractorCaffe over every rectangle of a set of frames:
    kind FACE (net builtin:FACE) or HAND (builtin:HAND); net_resolution = (w, h)."""

    def __init__(self, ctx, net, kind, net_resolution=(368, 368)):
        self.ctx = ctx
        self.L = ctx.L
        self.net = net
        self.kind = kind
        self.net_resolution = tuple(net_resolution)
        h = ctypes.c_void_p()
        check(self.L.opk_extractor_create(ctx.h, net.h, kind, net_resolution[0],
                                          net_resolution[1], ctypes.byref(h)))
        self.h = h
        _LIVE["extractor"].add(self)

    def close(self):
        if self.h:
            self.L.opk_extractor_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def parts(self):
        return self.L.opk_extractor_parts(self.h)

    def set_scales(self, number, rng=0.4):
        """--hand_scale_number / --hand_scale_range."""
        check(self.L.opk_extractor_set_scales(self.h, number, float(rng)))

    def set_max_batch(self, b):
        check(self.L.opk_extractor_set_max_batch(self.h, b))

    def set_heatmaps(self, scale_mode):
        """Per-person heat maps with op::ScaleMode scale_mode (-1 off; opk_extractor_set_heatmaps)."""
        check(self.L.opk_extractor_set_heatmaps(self.h, scale_mode))

    def heatmaps_numpy(self):
        """The last forward's heat maps: face [people, parts, H, W], hand [2, people, parts, H, W]."""
        p = ctypes.c_void_p()
        shape = (ctypes.c_int * 5)()
        check(self.L.opk_extractor_heatmaps(self.h, ctypes.byref(p), shape))
        dims = tuple(shape)
        out = np.zeros(dims, np.float32)
        if out.size:
            check(self.L.opk_memcpy_d2h(self.ctx.h, out.ctypes.data_as(ctypes.c_void_p), p,
                                        out.nbytes))
        return out[0] if self.kind == FACE else out

    def forward(self, frames, rectangles, frame_of=None):
        """frames: BGR uint8 [n, h, w, 3] CUDA tensor; rectangles [people, 4] (face) or
        [people, 2, 4] (hand); frame_of [people] or None.  Returns face [people, parts, 3] or
        hand [2, people, parts, 3] keypoints (numpy).  frames may be a Frames."""
        fs = _as_frames(frames).struct()
        r = np.ascontiguousarray(rectangles, np.float32)
        people = r.shape[0]
        hands = 2 if self.kind == HAND else 1
        out = np.zeros((hands, people, self.parts, 3), np.float32)
        fo = None
        if frame_of is not None:
            fo = np.ascontiguousarray(frame_of, np.int32)
            assert fo.shape == (people,)
        check(self.L.opk_extractor_forward_fmt(
            self.h, ctypes.byref(fs), r.ctypes.data_as(ctypes.c_void_p),
            fo.ctypes.data_as(ctypes.c_void_p) if fo is not None else None, people,
            out.ctypes.data_as(ctypes.c_void_p)))
        return out[0] if self.kind == FACE else out

    def crops(self):
        """[(2x3 inverse map, net input [3, h, w] numpy)] of the last forward's crops."""
        out = []
        w, h = self.net_resolution
        for i in range(self.L.opk_extractor_crop_count(self.h)):
            m = np.zeros(6, np.float64)
            p = ctypes.c_void_p()
            check(self.L.opk_extractor_crop(self.h, i, m.ctypes.data_as(ctypes.c_void_p),
                                            ctypes.byref(p)))
            x = None   # after a pose-pipeline stage run: the inputs are staged per net batch
            if p.value:
                x = np.empty((3, h, w), np.float32)
                check(self.L.opk_memcpy_d2h(self.ctx.h, x.ctypes.data_as(ctypes.c_void_p), p,
                                            x.nbytes))
            out.append((m.reshape(2, 3), x))
        return out
