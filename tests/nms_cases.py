"""The dense and tiny NMS cases (tests/test_nms_cases.py on the CPU, tests/test_gpu_nms_dense.py on
the GPU): input fields by name, the oracle's answers for them, and a numpy restatement of the two
peak tests that says at which pixels the peaks are.

Every field comes from a seeded numpy generator.  The merged maps and the oracle's peaks are
computed once per process and handed out read-only.

A  materialised maps (opk_nms): tiny maps, 128-256 and 513-1024 peaks per plane (one and several
   strides of the candidate sort), more than 1024, a mixed batch;
B  lazy maps (the pose pipeline on injected net outputs): source fields whose x8 maps hold
   128-256, 257-1024 and more than 1024 peaks per plane, a map narrower than one walk, a sparse
   field for the batch after an overflow.
"""
import functools

import numpy as np

import oracle
from oracle import parity
from tests.fields import noise_field, people_field

f32 = np.float32
TH = 0.05
OFFSET = (0.25, 0.5)      # the materialised cases' offsets
PARTS = 25
CAP1 = 128                # maxPeaks + 1 of the pipeline
FULL1 = 8192              # a capacity no case reaches: the oracle's untruncated answer
CANDIDATES = 1024         # kNmsCandidates (kernels.h): above it nms_finalize_kernel re-scans
PRODUCER = (1280, 720)
TINY = ((1, 1), (2, 3), (3, 3), (3, 4), (4, 5), (5, 4), (6, 7))
TINY_KINDS = ("uniform", "levels")


def _ro(a):
    a = np.ascontiguousarray(a, f32)
    a.setflags(write=False)
    return a


def uniform(shape, seed, lo=0.0):
    """i.i.d. uniform float32 noise in [lo, 1)"""
    u = np.random.default_rng(seed).random(shape, dtype=f32)
    return u if lo == 0.0 else u * f32(1.0 - lo) + f32(lo)


# ---- A: materialised maps ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiny(h, w, kind):
    """[25, h, w]: continuous noise, or 4-level quantised noise (plateaus everywhere)"""
    if kind == "uniform":
        return _ro(uniform((PARTS, h, w), 100 * h + w))
    return _ro(noise_field(PARTS, h, w, seed=h * 10 + w, levels=4, density=1.0))


@functools.lru_cache(maxsize=None)
def a2():
    """[2, 25, 40, 40]: 128-1024 peaks per plane"""
    return _ro(uniform((2, PARTS, 40, 40), 0))


@functools.lru_cache(maxsize=None)
def a3():
    """[1, 25, 120, 120]: more than 1024 peaks per plane"""
    return _ro(uniform((1, PARTS, 120, 120), 0))


@functools.lru_cache(maxsize=None)
def a4():
    """[2, 25, 100, 100]: frame 0 dense (A3 cropped), frame 1 three synthetic people"""
    return _ro(np.stack([a3()[0, :, :100, :100], people_field(3, 100, 100, seed=41)[:PARTS]]))


@functools.lru_cache(maxsize=None)
def a5():
    """[1, 25, 72, 72]: 513-1024 peaks per plane -- the candidate sort runs over more keys than
    the workgroup has lanes (several strides of the bitonic network)"""
    return _ro(uniform((1, PARTS, 72, 72), 1))


@functools.lru_cache(maxsize=None)
def materialised_reference(name, cuda, cap1=CAP1):
    """oracle.nms of every frame of a2 / a3 / a4 / a5: [frames, 25, cap1, 3]"""
    f = {"a2": a2, "a3": a3, "a4": a4, "a5": a5}[name]()
    return _ro(np.stack([oracle.nms(fr, TH, cap1, OFFSET, cuda=cuda) for fr in f]))


# ---- B: lazy maps through the pose pipeline ------------------------------------------------------
SOURCES = {"B1": (2, 23, 31), "B2": (1, 80, 120), "B3": (1, 5, 6), "B4": (1, 80, 120),
           "B5": (1, 45, 57)}


def _bumps(h, w, seed):
    """[78, h, w] sparse field: per part plane a two-pixel plateau of 0.5 on source columns 0 and 1
    (exact ties on the map's columns 0-3 under both resizes: a nmsCpu peak on column 1, none for
    nmsGpu), a bump falling off to 0.6 of its height on the next column (a strict maximum on map
    column 1 under the Catmull-Rom resize), one-pixel bumps in two corners and three inside;
    planes 13.. carry a little noise as well (no exact ties there)."""
    rng = np.random.default_rng(seed)
    f = np.zeros((78, h, w), f32)
    for c in range(PARTS):
        d = f32(0.004 * c)
        f[c, h - 2, 0] = f[c, h - 2, 1] = 0.5
        f[c, 1, 0] = f32(0.9) - d
        f[c, 1, 1] = f32(0.6) * f[c, 1, 0]
        f[c, 0, w - 1] = f32(0.6) + d
        f[c, h - 1, w - 1] = f32(0.4) + d
        f[c, 1, w // 2] = f32(0.8) - d
        f[c, 2, w // 2 + 1] = f32(0.3) + d
        f[c, h - 2, w // 2 + c % 2] = f32(0.65)
    f[13:PARTS] += rng.normal(0, 0.01, (PARTS - 13, h, w)).astype(f32)
    f[PARTS + 1:] = rng.uniform(-0.3, 0.3, (78 - PARTS - 1, h, w)).astype(f32)
    return f


@functools.lru_cache(maxsize=None)
def source(name):
    """[frames, 78, h, w] net output of a B case.  B1, B2, B5: uniform noise in [-0.2, 1); B3:
    hand-placed bumps; B4: the sparse batch that follows B2 on the same extractor."""
    n, h, w = SOURCES[name]
    if name in ("B1", "B2", "B5"):
        return _ro(uniform((n, 78, h, w), 2 if name == "B5" else 0, lo=-0.2))
    return _ro(np.stack([_bumps(h, w, seed=7 + k) for k in range(n)]))


def net_size(name):
    """(w, h) of the net input = of the heat maps (x8)"""
    _, h, w = SOURCES[name]
    return (8 * w, 8 * h)


def _scale_factor(init, target):
    """resizeGetScaleFactor (src/openpose/utilities/openCv.cpp:182-195)"""
    return min((target[0] - 1) / float(init[0] - 1), (target[1] - 1) / float(init[1] - 1))


def scale_net_to_output(name, producer=PRODUCER):
    """poseExtractorCaffe.cpp:281-310 for a net input of net_size(name)"""
    sp = _scale_factor(producer, net_size(name))
    net = (int(sp * producer[0] + 0.5), int(sp * producer[1] + 0.5))
    return f32(_scale_factor(net, producer))


def offset_of(scale):
    """the NMS offset the pipeline passes (poseExtractorCaffe.cpp:318), as the pipeline tests do"""
    return float(f32(0.5 / np.float64(scale)))


@functools.lru_cache(maxsize=None)
def heat(name, cuda):
    """[frames, 25, 8h, 8w]: the oracle's merged part maps of a B case under either resize"""
    w, h = net_size(name)
    fn = oracle.resize_merge_cuda if cuda else oracle.resize_merge
    return _ro(np.stack([fn([fr[:PARTS]], h, w) for fr in source(name)]))


@functools.lru_cache(maxsize=None)
def lazy_reference(name, cuda, off, cap1=CAP1):
    """oracle.nms of heat(name, cuda): [frames, 25, cap1, 3]"""
    return _ro(np.stack([oracle.nms(hm, TH, cap1, (off, off), cuda=cuda) for hm in heat(name, cuda)]))


# ---- where the peaks are -------------------------------------------------------------------------
def peak_mask(planes, cuda, th=TH):
    """Boolean [C, H, W]: nmsCpu's peak test (oracle/parity.py) or nmsRegisterKernel's
    (nmsBase.cu:50-90: interior pixels, value > threshold and > all 8 neighbours)."""
    planes = np.asarray(planes, f32)
    if not cuda:
        return parity.peak_mask(planes, th)
    c, h, w = planes.shape
    m = np.zeros((c, h, w), bool)
    if h < 3 or w < 3:
        return m
    v = planes[:, 1:-1, 1:-1]
    ok = v > f32(th)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                ok &= v > planes[:, dy:dy + h - 2, dx:dx + w - 2]
    m[:, 1:-1, 1:-1] = ok
    return m


def counts(planes, cuda):
    """the oracle's untruncated peak count of every plane"""
    return oracle.nms(planes, TH, FULL1, cuda=cuda, channels=planes.shape[0])[:, 0, 0].astype(int)
