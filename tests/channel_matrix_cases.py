"""The graphs, shapes and kernel instantiations of the channel matrix: output channel counts off
the grid of the shipped pose models ({16, 19, ..., 512}), at the smallest shapes that reach each
branch of the conv kernels.

Shared by tests/test_channel_matrix_plan.py (Net.conv_kernels on a host-only context: the planner
gives every case the instantiation it exists for) and tests/test_gpu_channel_matrix.py (the same
asserted from the launch log of a real forward, then every launch held to the per-launch bound of
tests/launch_check.py).

  offgrid  3x3 layers of 72, 100, 160 and 200 outputs (the 96- and 128-wide n-blocks with fewer
           channels, a partly empty last n-block), 1x1 layers of 384 and 768 (three 256-wide
           n-blocks), a 3x3 head of 19 fp32 outputs (the scalar net_output path of a 3x3) and a
           1x1 head of 65; also in small-batch mode (conv3s tiles with 8 and 32 valid channels)
  odd      members at the unaligned concat offsets 19, 57, 100 and 119, a conv stored to two
           concats and one stored to its own buffer and two concats, a 129-channel concat read
           as 160, 7x7 convs of 100 and 44 outputs
  head     the fused 1x1 head pair at n2 = 1, 32, 33 and 64, and the pairs that must run unfused
  first    the image conv with 4, 32 and 48 outputs
  pool     a stand-alone pool of 40, 72, 96 and 160 channels at odd sizes (ceil pooling)
"""
from tests.test_gpu_net import conv

CUS = 256   # the MI355X; the planner's answers below are for this chip


def _out(L, *members):
    L.append(dict(name="net_output", type="Concat", bottom=list(members), top=["net_output"]))
    return L


def offgrid_graph():
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 72, 3, "prelu")
    L += conv("c3", "c2", 100, 3, "relu") + conv("c4", "c3", 160, 3, "prelu")
    L += conv("c5", "c4", 200, 3, "prelu") + conv("c6", "c5", 384, 1, "prelu")
    L += conv("c7", "c6", 768, 1, "prelu") + conv("c8", "c7", 19, 3) + conv("c9", "c7", 65, 1)
    return _out(L, "c8", "c9")


def odd_graph():
    """`a` is stored to two concat slices (offsets 0 and 100), `c` to its own buffer (f reads it)
    and to the slices at 57 and 119; cat has 129 channels: cin_pad 160 with one live channel in the
    last chunk."""
    L = conv("c1", "image", 64, 3, "relu") + conv("a", "c1", 19, 3, "prelu") + conv("b", "c1", 38, 1)
    L += conv("c", "c1", 72, 3, "relu")
    L.append(dict(name="cat", type="Concat", bottom=["a", "b", "c"], top=["cat"]))
    L += conv("d", "cat", 100, 7, "prelu")
    L.append(dict(name="cat2", type="Concat", bottom=["d", "a", "c"], top=["cat2"]))
    L += conv("e", "cat2", 44, 7) + conv("f", "c", 15, 1)
    return _out(L, "e", "f")


def head_graph(n1, n2):
    L = conv("c1", "image", 64, 3, "relu") + conv("m6", "c1", n1, 1, "prelu") + conv("m7", "m6", n2, 1)
    return _out(L, "m7")


def first_graph(k):
    L = conv("c1", "image", k, 3, "relu") + conv("c2", "c1", 64, 3) + conv("c3", "c2", 26, 1)
    return _out(L, "c3")


def pool_graph(k):
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", k, 3, "relu")
    L.append(dict(name="p1", type="Pooling", bottom=["c2"], top=["p1"], pool="MAX", kernel_size=2,
                  stride=2))
    L += conv("c3", "p1", 64, 3, "prelu") + conv("c4", "c3", 26, 1)
    return _out(L, "c4")


def instantiation(kernel, prefix, split):
    """Is `kernel` (a launch-log or conv_kernels name) the instantiation `prefix` -- its template
    arguments up to the precision -- in the given precision?  Bare kernels (conv_image_kernel,
    conv_head_kernel, conv_head_kernel<256,2,) match by prefix."""
    if "<" not in prefix or prefix.endswith(","):
        return kernel.startswith(prefix) and ("split" in kernel) == (split and "<" in kernel)
    if split:
        return kernel in (prefix + ",split>", prefix + ",8,split>")
    return kernel == prefix + ">"


def case(name, graph, shape, split, small=False, must_run=None, args=()):
    """must_run: {conv: instantiation prefix, or None for a conv that runs inside the kernel of the
    conv before it}."""
    return dict(name="%s %dx%dx%d %s%s" % ((name, ) + tuple(shape) + ("split" if split else "fp16",
                                                                      " small" if small else "")),
                graph=graph, args=tuple(args), shape=tuple(shape), split=split, small=small,
                must_run=dict(must_run or {}))


# ---- 1, 2: off-grid outputs --------------------------------------------------------------------

OFFGRID_SMALL_SHAPE = {
    (2, 24, 40): dict(c2="conv3_kernel<256,96,512,3,1,3", c3="conv3_kernel<256,128,512,3,1,3",
                      c4="conv3_kernel<256,128,512,3,1,3", c5="conv3_kernel<256,128,512,3,1,3",
                      c6="conv3_kernel<256,128,256,1,2,1", c7="conv3_kernel<256,256,256,1,1,1,16",
                      c8="conv3_kernel<512,64,768,3,1,3", c9="conv3_kernel<256,96,256,1,2,1"),
    # exactly 768 tiles of 256 positions for two n-blocks: the 16-wave tile with a 32-channel (c4)
    # and a 72-channel (c5) last n-block
    (48, 62, 30): dict(c4="conv3_kernel<512,128,704,3,1,3,16", c5="conv3_kernel<512,128,704,3,1,3,16",
                       c7="conv3_kernel<256,256,256,1,1,1,16"),
}
assert 48 * (62 + 2) * (30 + 2) // 256 * 2 == 768

OFFGRID_SMALL_MODE = {
    (1, 24, 40): {n: "conv3s_kernel<64,32,256,9" for n in ("c2", "c3", "c4", "c5", "c8")},
    # 128 x 64 tiles: last tiles of 32 (160 = 2 * 64 + 32) and 8 (200 = 3 * 64 + 8) valid channels
    (1, 62, 126): dict(c4="conv3s_kernel<128,64,320,3", c5="conv3s_kernel<128,64,320,3"),
}


def offgrid_cases():
    out = []
    for shape, must in OFFGRID_SMALL_SHAPE.items():
        for split in (False, True):
            out.append(case("offgrid", offgrid_graph, shape, split, must_run=must))
    return out


def offgrid_small_cases():
    out = []
    for shape, must in OFFGRID_SMALL_MODE.items():
        for split in (False, True):
            out.append(case("offgrid", offgrid_graph, shape, split, small=True, must_run=must))
    return out


# ---- 3: odd concats and 7x7 ---------------------------------------------------------------------

def odd_cases():
    must = dict(d="conv3_kernel<256,128,1024,1,1,7", e="conv3_kernel<256,64,1024,1,1,7")
    out = [case("odd", odd_graph, (2, 24, 40), split, must_run=must) for split in (False, True)]
    small = dict(d="conv3s_kernel<64,32,384,7,7", e="conv3s_kernel<64,32,384,7,7",
                 a="conv3s_kernel<64,32,256,9", c="conv3s_kernel<64,32,256,9")
    out.append(case("odd", odd_graph, (1, 46, 46), False, small=True, must_run=small))
    return out


# ---- 4: fused heads -----------------------------------------------------------------------------

FUSED_HEADS = [(256, 1, False), (256, 32, False), (256, 33, False), (256, 33, True), (512, 64, False)]
UNFUSED_HEADS = {(512, 65): dict(m6="conv3_kernel<256,256,256,1,1,1,16", m7="conv3_kernel<256,96,256,1,2,1"),
                 (128, 26): dict(m6="conv3_kernel<256,128,256,1,2,1", m7="conv3_kernel<256,64,256,1,2,1"),
                 (384, 26): dict(m6="conv3_kernel<256,128,256,1,2,1", m7="conv3_kernel<256,64,256,1,2,1")}


def head_cases():
    out = []
    for n1, n2, split in FUSED_HEADS:
        # (the launch log adds the instantiation: <n1, n2p / 16, persistent, max-epilogue>)
        out.append(case("head %d-%d" % (n1, n2), head_graph, (2, 24, 40), split, args=(n1, n2),
                        must_run=dict(m6="conv_head_kernel", m7=None)))
    for (n1, n2), must in UNFUSED_HEADS.items():
        out.append(case("head %d-%d" % (n1, n2), head_graph, (2, 24, 40), False, args=(n1, n2),
                        must_run=must))
    return out


def head_log_prefix(n1, n2):
    """The launch-log name of the fused pair: the 32- or 64-wide Mconv7 tile (NF2 = 2 or 4)."""
    return "conv_head_kernel<%d,%d," % (n1, 2 if n2 <= 32 else 4)


# ---- 5: the first conv --------------------------------------------------------------------------

FIRST_OUTPUTS = (4, 32, 48)
FIRST_REFUSED = (6, 96)   # not a multiple of 4; more than 64: refused at construction


def first_cases():
    return [case("first %d" % k, first_graph, (2, 24, 40), split, args=(k, ),
                 must_run=dict(c1="conv_image_kernel", c2="conv3_kernel<512,64,768,3,1,3"))
            for k in FIRST_OUTPUTS for split in (False, True)]


# ---- 6: a stand-alone pool of off-grid channels -------------------------------------------------

POOL_CHANNELS = {40: "conv3_kernel<512,64,768,3,1,3", 72: "conv3_kernel<256,96,512,3,1,3",
                 96: "conv3_kernel<256,96,512,3,1,3", 160: "conv3_kernel<256,128,512,3,1,3"}


def pool_cases():
    return [case("pool %d" % k, pool_graph, (2, 25, 41), split, args=(k, ), must_run=dict(c2=inst))
            for k, inst in POOL_CHANNELS.items() for split in (False, True)]


def all_cases():
    out = offgrid_cases() + offgrid_small_cases() + odd_cases() + head_cases() + first_cases() + pool_cases()
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names), names
    return out
