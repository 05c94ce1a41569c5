"""GPU parity of the BODY_25 CNN (NetHip, MFMA fp16 / fp32 accumulate) vs the fp32 Caffe-semantics
oracle (oracle/caffe_cpu.c) on identical inputs and seeded weights.

Tolerance (floating point, north_star: outputs within a stated float tolerance): fp16 operands give
~2^-11 relative rounding per operand; the bar below is relative L2 error of the net output.
"""
import os
import tempfile

import numpy as np
import pytest
import torch

import oracle
from oracle import body25
from openpose_amd import synth
from openpose_amd.api import Net, dev_switches
from tests import prototxt

pytestmark = pytest.mark.gpu

SMALL_TOL = 4e-3      # relative L2, graphs of <= 6 layers
BODY25_TOL = 5e-3     # relative L2, the full 114-conv network (measured 1.5-2.5e-3)
CHANNEL_TOL = 2e-2    # relative L2 of any single output channel of a frame (measured < 6e-3)


def rel_l2(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30))


def conv(name, bottom, cout, k, act=None):
    out = [dict(name=name, type="Convolution", bottom=[bottom], top=[name], num_output=cout,
                kernel_size=k, pad=k // 2)]
    if act:
        out.append(dict(name=act + "_" + name, type="ReLU" if act == "relu" else "PReLU",
                        bottom=[name], top=[name]))
    return out


def run_graph(ctx, layers, x, seed=0, precision=None):
    text = prototxt.emit(layers)
    graph = prototxt.parse(text)
    params = synth.he_weights(graph, seed=seed)
    with tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False) as f:
        f.write(text)
        path = f.name
    try:
        net = Net(ctx, path)
        net.set_params(params)
        if precision is not None:
            net.set_precision(precision)
        net.forward(torch.from_numpy(x).cuda())
        got = net.output_numpy()
        net.close()
    finally:
        os.unlink(path)
    ref = body25.forward(x, params, graph=graph)
    return got, ref


def test_conv_relu_prelu_1x1(ctx):
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 96, 3, "prelu") + conv("c3", "c2", 52, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["c3"], top=["net_output"]))
    x = np.random.default_rng(0).uniform(-0.5, 0.5, (2, 3, 24, 40)).astype(np.float32)
    got, ref = run_graph(ctx, L, x)
    assert got.shape == ref.shape
    assert rel_l2(got, ref) < SMALL_TOL


def test_dense_block_concat_and_pool(ctx):
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 128, 3, "relu")
    L.append(dict(name="p1", type="Pooling", bottom=["c2"], top=["p1"], kernel_size=2, stride=2))
    L += conv("c3", "p1", 128, 3, "prelu")
    L += conv("a0", "c3", 96, 3, "prelu") + conv("a1", "a0", 96, 3, "prelu") + conv("a2", "a1", 96, 3, "prelu")
    L.append(dict(name="cat", type="Concat", bottom=["a0", "a1", "a2"], top=["cat"]))
    L += conv("m6", "cat", 256, 1, "prelu") + conv("m7", "m6", 26, 1)
    L.append(dict(name="cat2", type="Concat", bottom=["c3", "m7"], top=["cat2"]))
    L += conv("b0", "cat2", 128, 3, "prelu") + conv("b7", "b0", 52, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["m7", "b7"], top=["net_output"]))
    # odd sizes exercise Caffe's ceil pooling
    x = np.random.default_rng(1).uniform(-0.5, 0.5, (3, 3, 37, 51)).astype(np.float32)
    got, ref = run_graph(ctx, L, x)
    assert got.shape == ref.shape == (3, 78, 19, 26)
    assert rel_l2(got, ref) < SMALL_TOL


@pytest.mark.parametrize("n,h,w", [(2, 64, 96), (1, 368, 368)])
def test_body25_vs_oracle(ctx, n, h, w):
    graph = body25.layers()
    params = synth.he_weights(graph, seed=3)
    x = np.random.default_rng(4).uniform(-0.5, 0.5, (n, 3, h, w)).astype(np.float32)
    net = Net(ctx, "builtin:BODY_25")
    net.set_params(params)
    net.forward(torch.from_numpy(x).cuda())
    got = net.output_numpy()
    ref = body25.forward(x, params, graph=graph)
    assert got.shape == ref.shape == (n, 78, h // 8, w // 8)
    err = rel_l2(got, ref)
    print("BODY_25 %dx%dx%d rel-L2 %.3e" % (n, h, w, err))
    assert err < BODY25_TOL


def ch_ok(got, ref):
    return channel_errors(got, ref).max() < CHANNEL_TOL


def channel_errors(got, ref):
    """relative L2 per (frame, channel) plane"""
    d = np.linalg.norm((got - ref).reshape(got.shape[0], got.shape[1], -1), axis=2)
    r = np.linalg.norm(ref.reshape(ref.shape[0], ref.shape[1], -1), axis=2)
    return d / np.maximum(r, 1e-30)


def test_body25_bench_geometry_vs_oracle(ctx):
    """The net at the bench's shape (the tile-aligned batch of bench.py -- 130 x 3 x 368 x 656 on a
    256-CU MI355X: the persistent stage-layer kernels, the 8-wave VGG / pooled kernels, the fused
    heads and conv1, with the bench's grids and tile walk), frames 0, the middle one and the last
    (first, middle and last tile rounds) against the fp32 oracle, whole-frame and per-channel
    tolerance; and against the fp16-storage emulation (oracle/fp16.py: what the kernels compute up
    to the fp32 summation order), within the same tolerance.  Layer-by-layer bounds:
    tests/test_gpu_layers.py."""
    from bench import tile_aligned_batch
    from oracle import fp16 as emu
    graph = body25.layers()
    params = synth.he_weights(graph, seed=13)
    n = tile_aligned_batch(torch.cuda.get_device_properties(0).multi_processor_count)
    h, w = 368, 656
    rng = np.random.default_rng(14)
    x = rng.uniform(-0.5, 0.5, (n, 3, h, w)).astype(np.float32)
    net = Net(ctx, "builtin:BODY_25")
    net.set_params(params)
    net.forward(torch.from_numpy(x).cuda())
    got = net.output_numpy()
    assert got.shape == (n, 78, h // 8, w // 8)
    pick = [0, n // 2 - 1, n - 1]
    ref = body25.forward(x[pick], params, graph=graph)
    err = rel_l2(got[pick], ref)
    ch = channel_errors(got[pick], ref)
    ref16 = emu.forward(x[pick], params, graph)
    err16 = rel_l2(got[pick], ref16)
    print("BODY_25 %dx368x656 frames %s rel-L2 %.3e (fp32 oracle), %.3e (fp16-storage emulation), "
          "worst channel %.3e" % (n, pick, err, err16, ch.max()))
    assert err < BODY25_TOL
    assert ch.max() < CHANNEL_TOL
    # the emulation is NOT closer at the whole-net level (measured 2.15e-3 vs 2.22e-3): last-bit
    # differences of each layer's summation order propagate through ~100 layers; the per-layer
    # bounds of tests/test_gpu_layers.py are the tight check
    assert err16 < BODY25_TOL


def test_net_output_query_follows_addCaffeNetOnThread(ctx):
    """The call sequence PoseExtractorCaffe uses (poseExtractorCaffe.cpp:82-95): create the net,
    query its output blob BEFORE any forward (it is kept for every frame), forward, read it,
    forward again: the blob of one input shape keeps its device pointer and holds the new
    values (NetCaffe's live blob, netCaffe.cpp:263-268)."""
    graph = body25.layers()
    params = synth.he_weights(graph, seed=15)
    net = Net(ctx, "builtin:BODY_25")
    p0, shape0 = net.output()
    assert p0 is None and shape0 == (0, 78, 0, 0)
    net.set_params(params)
    rng = np.random.default_rng(16)
    x1 = rng.uniform(-0.5, 0.5, (2, 3, 64, 96)).astype(np.float32)
    x2 = rng.uniform(-0.5, 0.5, (2, 3, 64, 96)).astype(np.float32)
    net.forward(torch.from_numpy(x1).cuda())
    p1, shape1 = net.output()
    v1 = net.output_numpy()
    net.forward(torch.from_numpy(x2).cuda())
    p2, shape2 = net.output()
    v2 = net.output_numpy()
    assert p1 is not None and p1 == p2 and shape1 == shape2 == (2, 78, 8, 12)
    assert not np.array_equal(v1, v2)
    ref2 = body25.forward(x2, params, graph=graph)
    assert rel_l2(v2, ref2) < BODY25_TOL


@pytest.mark.parametrize("hw,acts", [((24, 40), ("relu", "relu")), ((26, 130), ("relu", "prelu")),
                                     ((14, 6), ("prelu", "relu"))])
def test_conv1_fused_matches_unfused(ctx, hw, acts):
    """conv1_1 -> conv1_2 -> pool1 in one kernel (conv1_fused.hip) gives the bits of the three
    separate kernels (same MFMA operands and accumulation order, same epilogue, same max)."""
    L = conv("c1", "image", 64, 3, acts[0]) + conv("c2", "c1", 64, 3, acts[1])
    L.append(dict(name="pool1", type="Pooling", bottom=["c2"], top=["pool1"], pool="MAX",
                  kernel_size=2, stride=2))
    L += conv("c3", "pool1", 32, 3, "relu") + conv("c4", "c3", 16, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["c4"], top=["net_output"]))
    x = np.random.default_rng(7).uniform(-0.5, 0.5, (3, 3) + hw).astype(np.float32)
    outs = []
    for fused in (1, 0):
        with dev_switches(CONV1_FUSED=fused):
            got, ref = run_graph(ctx, L, x, seed=3)
        assert rel_l2(got, ref) < SMALL_TOL
        outs.append(got)
    np.testing.assert_array_equal(outs[0], outs[1])


def cpm_stage_graph(out_is_concat=True):
    """A COCO / hand-like CPM net in miniature: VGG 3x3 front with a pool, then two refinement
    stages of 7x7 (pad 3) convs on concat(features, previous stage), 1x1 heads; the whole net
    gets a 3-pixel zero border."""
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 64, 3, "relu")
    L.append(dict(name="p1", type="Pooling", bottom=["c2"], top=["p1"], pool="MAX",
                  kernel_size=2, stride=2))
    L += conv("c3", "p1", 128, 3, "relu") + conv("feat", "c3", 96, 3, "relu")
    L += conv("s1a", "feat", 128, 3, "relu") + conv("s1b", "s1a", 64, 1, "relu") + conv("s1", "s1b", 22, 1)
    L.append(dict(name="cat2", type="Concat", bottom=["s1", "feat"], top=["cat2"]))
    L += conv("s2a", "cat2", 128, 7, "relu") + conv("s2b", "s2a", 128, 7, "relu")
    L += conv("s2c", "s2b", 96, 7, "relu") + conv("s2d", "s2c", 128, 1, "relu")
    if out_is_concat:
        L += conv("s2", "s2d", 19, 1) + conv("s2p", "s2d", 38, 1)
        L.append(dict(name="net_output", type="Concat", bottom=["s2", "s2p"], top=["net_output"]))
    else:   # the hand / face nets: the last conv's top is the output blob
        L += [dict(name="s2", type="Convolution", bottom=["s2d"], top=["net_output"], num_output=22,
                   kernel_size=1, pad=0)]
    return L


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("hw", [(64, 96), (96, 200)])
def test_7x7_cpm_stages_vs_oracle(ctx, concat, hw):
    x = np.random.default_rng(21).uniform(-0.5, 0.5, (2, 3) + hw).astype(np.float32)
    got, ref = run_graph(ctx, cpm_stage_graph(concat), x, seed=5)
    err = rel_l2(got, ref)
    print("7x7 CPM %s rel-L2 %.3e" % (hw, err))
    assert got.shape == ref.shape and err < SMALL_TOL


VARIANTS = {k: dict(v) for k, v in {
    "persistent": {}, "persistent_conv3p": {"CONV3W": 0}, "w16": {"CONV3_PERSIST": 0},
    "persistent_8wave": {"CONV3W8": 2}, "persistent_no_8wave": {"CONV3W8": 0},
    "w8": {"CONV3_W16": 0, "CONV1_TILE": 0}, "w8_one_per_cu": {"CONV3_W16": 0, "CONV3_SMALL": 0},
    "persistent_compiler_frags": {"CONV3W": 0, "CONV3P_ASMR": 0},
    "persistent_dwordx2": {"CONV3W": 0, "CONV3P_WIDE": 0},
    "dwordx2": {"CONV3W": 0, "CONV3P_WIDE": 0, "CONV3_WIDE": 0},
    "w16_dwordx2": {"CONV3_PERSIST": 0, "CONV3_WIDE": 0},
    "conv1_512x128": {"CONV1_TILE": 1}, "conv1_256x256": {"CONV1_TILE": 2},
    "conv1_512x64": {"CONV1_N64W16": 1},
    "nblocks_16wave": {"CONV3W8N": 0},
    "epilogue_select": {"EPI_MAX": 0}, "w8_epilogue_select": {"CONV3W8": 2, "EPI_MAX": 0},
    "w8_all": {"CONV3W8": 3}, "head_per_tile": {"HEAD_PERSIST": 0},
    "pointer_stores": {"BUFST": 0}, "w8_pointer_stores": {"CONV3W8": 2, "BUFST": 0},
    # (the graph below has no eligible 64-output 3x3 layer: names the switch; its A/B is
    # tests/test_gpu_launch_matrix.py::test_ab_variants_bit_identical)
    "w8_64_off": {"CONV3W8_64": 0}}.items()}
ROUNDING_VARIANTS = set()   # variants with another MFMA shape (another fp32 summation order)


def test_conv3_tile_variants_bit_identical(ctx):
    """The conv3 tile variants (persistent 16-wave 512-row tiles, 16-wave, 8-wave 256-row tiles
    one or two per CU) feed the MFMAs the same operands in the same K order, so the net output is
    bit-identical whichever runs; the 8-wave ones are pinned to the oracle by the tests above.
    2 x 256 x 384 makes >= 768 tiles per 128/96-channel layer, the 16-wave threshold."""
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 128, 3, "relu")
    L += conv("c3", "c2", 96, 3, "prelu") + conv("c4", "c3", 128, 3, "prelu")
    L += conv("c5", "c4", 96, 3, "relu")
    L.append(dict(name="cat", type="Concat", bottom=["c3", "c5"], top=["cat"]))
    L += conv("c6", "cat", 128, 3, "prelu") + conv("c6b", "c6", 256, 3, "relu")
    L += conv("c6d", "c6b", 512, 3, "prelu")   # 2 and 4 n-blocks of 128 (conv3w8 n-block grid)
    L += conv("c6c", "c6d", 512, 1, "prelu") + conv("c7", "c6c", 52, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["c7"], top=["net_output"]))
    text = prototxt.emit(L)
    graph = prototxt.parse(text)
    params = synth.he_weights(graph, seed=11)
    x = np.random.default_rng(12).uniform(-0.5, 0.5, (2, 3, 256, 384)).astype(np.float32)
    with tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False) as f:
        f.write(text)
        path = f.name
    outs = {}
    try:
        for name, sw in VARIANTS.items():
            with dev_switches(**sw):
                net = Net(ctx, path)
                net.set_params(params)
                net.forward(torch.from_numpy(x).cuda())
                outs[name] = net.output_numpy()
                net.close()
    finally:
        os.unlink(path)
    assert np.isfinite(outs["w8"]).all() and np.abs(outs["w8"]).max() > 0
    for name in VARIANTS:
        if name in ROUNDING_VARIANTS:   # other MFMA shape: another fp32 summation order
            assert rel_l2(outs[name], outs["w8"]) < 1e-3, name
            continue
        np.testing.assert_array_equal(outs[name], outs["w8"], err_msg=name)
    # and the fp32 torch restatement of the same graph agrees within the fp16 tolerance
    ref = torch_forward(graph, params, x)
    assert rel_l2(outs["persistent"], ref) < SMALL_TOL and ch_ok(outs["persistent"], ref)


def torch_forward(graph, params, x):
    """fp32 torch (CPU) evaluation of a conv/ReLU/PReLU/Concat graph (test_gpu_net graphs only)."""
    import torch.nn.functional as F
    blobs = {"image": torch.from_numpy(x)}
    producer = {}
    for l in graph:
        t = l["type"]
        if t == "Convolution":
            producer[l["top"][0]] = l["name"]
            w, b = params[l["name"]][:2]
            blobs[l["top"][0]] = F.conv2d(blobs[l["bottom"][0]], torch.from_numpy(np.asarray(w)),
                                          torch.from_numpy(np.asarray(b)), padding=l.get("pad", 0))
        elif t == "ReLU":
            blobs[l["top"][0]] = torch.relu(blobs[l["bottom"][0]])
        elif t == "PReLU":
            s = torch.from_numpy(np.asarray(params[producer[l["bottom"][0]]][2]))
            blobs[l["top"][0]] = F.prelu(blobs[l["bottom"][0]], s)
        elif t == "Concat":
            blobs[l["top"][0]] = torch.cat([blobs[b] for b in l["bottom"]], 1)
        elif t == "Pooling":   # Caffe MAX 2x2 / 2, ceil sizing
            blobs[l["top"][0]] = F.max_pool2d(blobs[l["bottom"][0]], 2, 2, ceil_mode=True)
    return blobs["net_output"].numpy()


def torch_forward64(graph, params, x):
    """float64 torch (CPU) evaluation of the same graph: the exact result the fp32 paths
    approximate (test_body25_split_precision_vs_oracle)."""
    import torch.nn.functional as F
    d = torch.float64
    blobs = {"image": torch.from_numpy(np.asarray(x, np.float64))}
    producer = {}
    for l in graph:
        t = l["type"]
        if t == "Convolution":
            producer[l["top"][0]] = l["name"]
            w, b = params[l["name"]][:2]
            blobs[l["top"][0]] = F.conv2d(blobs[l["bottom"][0]], torch.from_numpy(np.asarray(w)).to(d),
                                          torch.from_numpy(np.asarray(b)).to(d), padding=l.get("pad", 0))
        elif t == "ReLU":
            blobs[l["top"][0]] = torch.relu(blobs[l["bottom"][0]])
        elif t == "PReLU":
            s = torch.from_numpy(np.asarray(params[producer[l["bottom"][0]]][2])).to(d)
            blobs[l["top"][0]] = F.prelu(blobs[l["bottom"][0]], s)
        elif t == "Concat":
            blobs[l["top"][0]] = torch.cat([blobs[b] for b in l["bottom"]], 1)
        elif t == "Pooling":
            blobs[l["top"][0]] = F.max_pool2d(blobs[l["bottom"][0]], 2, 2, ceil_mode=True)
    return blobs["net_output"].numpy()


@pytest.mark.parametrize("name,hw", [("builtin:COCO_18", (64, 96)), ("builtin:MPI_15_4", (48, 80)),
                                     ("builtin:HAND", (64, 64)), ("builtin:FACE", (48, 64))])
def test_reference_cpm_nets_vs_oracle(ctx, name, hw):
    """The reference's other networks (7x7 stages, 3-pixel border, ReLU) against the fp32 oracle
    on the same seeded weights; graphs from tests/cpm_graphs.py (= the reference prototxts,
    tests/test_models.py)."""
    from tests import cpm_graphs
    graph = prototxt.parse(prototxt.emit(cpm_graphs.GRAPHS[name]()))
    params = synth.he_weights(graph, seed=9)
    x = np.random.default_rng(10).uniform(-0.5, 0.5, (2, 3) + hw).astype(np.float32)
    net = Net(ctx, name)
    net.set_params(params)
    net.forward(torch.from_numpy(x).cuda())
    got = net.output_numpy()
    net.close()
    ref = body25.forward(x, params, graph=graph)
    err = rel_l2(got, ref)
    print("%s %s rel-L2 %.3e" % (name, hw, err))
    assert got.shape == ref.shape and err < BODY25_TOL


def test_coco_pose_pipeline_runs_on_the_net(ctx):
    """COCO_18 end to end: frames -> warp -> COCO net -> lazy resize -> NMS -> connector, equal to
    feeding the same net output through the injection path."""
    from openpose_amd.api import PoseExtractor
    from openpose_amd.pose_tables import COCO_18
    from tests import cpm_graphs
    graph = prototxt.parse(prototxt.emit(cpm_graphs.GRAPHS["builtin:COCO_18"]()))
    net = Net(ctx, "builtin:COCO_18")
    net.set_params(synth.he_weights(graph, seed=2, out_scale=0.02))
    pose = PoseExtractor(ctx, net, pose_model=COCO_18)
    pose.set_input((-1, 96))
    frames = torch.randint(0, 256, (2, 90, 160, 3), dtype=torch.uint8)
    pose.forward_frames(frames.cuda())
    got = [pose.keypoints(f) for f in range(2)]
    out = torch.from_numpy(net.output_numpy()).cuda()
    ref = PoseExtractor(ctx, None, pose_model=COCO_18)
    ref.forward_net_output(out, (out.shape[3] * 8, out.shape[2] * 8), (160, 90))
    for f in range(2):
        kp, ks = ref.keypoints(f)
        np.testing.assert_array_equal(got[f][0], kp)
        np.testing.assert_array_equal(got[f][1], ks)
    assert pose.peaks_numpy().shape[1] == 18


@pytest.mark.parametrize("precision", ["fp16", "split"])
def test_conv_image_store_paths_bit_identical(ctx, precision):
    """conv_image's three store paths -- 16-byte pieces staged per wave in LDS and stored as whole
    pixels (the default), 16-byte pieces stored directly (CONV_IMAGE_STAGE=0) and 8-byte stores
    (CONV_IMAGE_WIDE=0) -- write the same conv1_1 blob (hi and, split, lo) and the same net output,
    on a width that leaves a partial 64-column tile (656 = 10 x 64 + 16)."""
    from openpose_amd.api import PRECISION_SPLIT
    graph = body25.layers()
    params = synth.he_weights(graph, seed=61)
    x = np.random.default_rng(62).uniform(-0.5, 0.5, (2, 3, 64, 656)).astype(np.float32)
    outs = {}
    for name, sw in {"stage": {}, "direct": {"CONV_IMAGE_STAGE": 0}, "narrow": {"CONV_IMAGE_WIDE": 0}}.items():
        with dev_switches(CONV1_FUSED=0, LAUNCH_LOG=1, **sw):
            net = Net(ctx, "builtin:BODY_25")
            net.set_params(params)
            if precision == "split":
                net.set_precision(PRECISION_SPLIT)
            net.forward(torch.from_numpy(x).cuda())
            assert any(k.startswith("conv_image_kernel") for _, k in net.launch_log())
            outs[name] = (net.blob("conv1_1"), net.output_numpy())
            net.close()
    assert np.abs(outs["stage"][0]).max() > 0
    for name in ("direct", "narrow"):
        np.testing.assert_array_equal(outs["stage"][0], outs[name][0])
        np.testing.assert_array_equal(outs["stage"][1], outs[name][1])


@pytest.mark.parametrize("precision", ["fp16", "split"])
def test_head_fusion_matches_unfused_and_oracle(ctx, precision):
    """Mconv6 -> Mconv7 pairs (1x1 to 512 / 256 channels, then 1x1 to <= 64) run as one
    conv_head_kernel: fp16 outputs into a concat read by a later conv and fp32 net-output channels.
    Against the two conv3 launches (HEAD_FUSE=0) only the fp32 summation order of Mconv7 differs
    (per-wave partials summed in a fixed order); against the fp32 oracle the usual tolerance.
    Split precision: conv_head's split instantiations (Mconv6's value split into the pair the
    unfused layer stores) against the unfused split pair and the oracle at the split tolerance."""
    from openpose_amd.api import PRECISION_SPLIT
    split = precision == "split"
    L = conv("c0", "image", 64, 3, "relu") + conv("c1", "c0", 96, 3, "prelu")
    L += conv("m6", "c1", 512, 1, "prelu") + conv("m7", "m6", 52, 1)
    L += conv("n6", "c1", 256, 1, "relu") + conv("n7", "n6", 26, 1)
    L.append(dict(name="cat", type="Concat", bottom=["m7", "c1"], top=["cat"]))
    L += conv("c2", "cat", 32, 3, "relu")
    L.append(dict(name="net_output", type="Concat", bottom=["n7", "m7", "c2"], top=["net_output"]))
    text = prototxt.emit(L)
    graph = prototxt.parse(text)
    params = synth.he_weights(graph, seed=21)
    x = np.random.default_rng(22).uniform(-0.5, 0.5, (3, 3, 96, 160)).astype(np.float32)
    with tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False) as f:
        f.write(text)
        path = f.name
    outs = {}
    try:
        for name, sw in {"fused": {}, "unfused": {"HEAD_FUSE": 0}}.items():
            with dev_switches(LAUNCH_LOG=1, **sw):
                net = Net(ctx, path)
                net.set_params(params)
                if split:
                    net.set_precision(PRECISION_SPLIT)
                net.forward(torch.from_numpy(x).cuda())
                outs[name] = net.output_numpy()
                heads = [k for _, k in net.launch_log() if k.startswith("conv_head")]
                assert len(heads) == (2 if name == "fused" else 0), heads
                assert all(k.endswith(",split>") == split for k in heads), heads
                net.close()
    finally:
        os.unlink(path)
    ref = body25.forward(x, params, graph=graph)
    if split:
        d, e = rel_l2(outs["fused"], outs["unfused"]), rel_l2(outs["fused"], ref)
        print("split heads: fused vs unfused rel-L2 %.3e, vs the fp32 oracle %.3e" % (d, e))
        assert d < 1e-6 and e < SPLIT_TOL
        assert channel_errors(outs["fused"], ref).max() < SPLIT_CHANNEL_TOL
        return
    assert rel_l2(outs["fused"], outs["unfused"]) < 1e-4
    assert rel_l2(outs["fused"], ref) < SMALL_TOL
    for c in range(ref.shape[1]):
        assert rel_l2(outs["fused"][:, c], ref[:, c]) < CHANNEL_TOL, c


def test_pool_fused_epilogue_bit_identical(ctx):
    """2x2 max pools fused into the epilogue of the conv that alone feeds them (conv3w8 POOL:
    pool2 / pool3 of BODY_25, pose_deploy.prototxt:70-87,149-166) are bit-identical to the separate
    pool kernel: one 128-channel and one 256-channel (2 n-block) conv, 8 x 368 x 328 (persistent
    tiles, even 82-column strips at both levels)."""
    L = conv("c1", "image", 64, 3, "relu") + conv("c2", "c1", 128, 3, "relu")
    L.append(dict(name="p1", type="Pooling", bottom=["c2"], top=["p1"], kernel_size=2, stride=2))
    L += conv("c3", "p1", 256, 3, "relu")
    L.append(dict(name="p2", type="Pooling", bottom=["c3"], top=["p2"], kernel_size=2, stride=2))
    L += conv("c4", "p2", 52, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["c4"], top=["net_output"]))
    text = prototxt.emit(L)
    graph = prototxt.parse(text)
    params = synth.he_weights(graph, seed=17)
    x = np.random.default_rng(18).uniform(-0.5, 0.5, (8, 3, 368, 328)).astype(np.float32)
    with tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False) as f:
        f.write(text)
        path = f.name
    outs = {}
    try:
        for name, fuse in (("fused", 1), ("separate", 0)):
            with dev_switches(POOL_FUSE=fuse):
                net = Net(ctx, path)
                net.set_params(params)
                net.forward(torch.from_numpy(x).cuda())
                outs[name] = net.output_numpy()
                net.close()
    finally:
        os.unlink(path)
    assert np.abs(outs["fused"]).max() > 0
    np.testing.assert_array_equal(outs["fused"], outs["separate"])
    ref = torch_forward(graph, params, x[:2])
    assert rel_l2(outs["fused"][:2], ref) < SMALL_TOL


def test_prelu_slopes_outside_unit_interval(ctx):
    """The epilogues use max(t, t*m) only when every negative-side multiplier of a conv lies in
    [0, 1] (ConvArgs::actmax, set per conv from its slopes); trained PReLU slopes may not.  With
    slopes drawn from [-0.5, 1.5] every conv falls back to the select, through conv1_fused, the
    persistent stage kernels and the pool-fused conv3w8: the fp32 reference is met and the result
    equals the EPI_MAX=0 build bit for bit."""
    L = conv("c1", "image", 64, 3, "prelu") + conv("c2", "c1", 64, 3, "prelu")
    L.append(dict(name="p1", type="Pooling", bottom=["c2"], top=["p1"], pool="MAX", kernel_size=2, stride=2))
    L += conv("c3", "p1", 128, 3, "prelu") + conv("c4", "c3", 128, 3, "prelu")
    L.append(dict(name="p2", type="Pooling", bottom=["c4"], top=["p2"], pool="MAX", kernel_size=2, stride=2))
    L += conv("c5", "p2", 128, 3, "prelu") + conv("c6", "c5", 96, 3, "prelu") + conv("c7", "c6", 52, 1)
    L.append(dict(name="net_output", type="Concat", bottom=["c7"], top=["net_output"]))
    text = prototxt.emit(L)
    graph = prototxt.parse(text)
    params = synth.he_weights(graph, seed=41)
    rng = np.random.default_rng(42)
    wild = 0
    for name, (w, b, s) in list(params.items()):
        if s is not None:
            s = rng.uniform(-0.5, 1.5, s.shape).astype(np.float32)
            wild += int(((s < 0) | (s > 1)).any())
            params[name] = (w, b, s)
    assert wild >= 5
    x = rng.uniform(-0.5, 0.5, (2, 3, 368, 656)).astype(np.float32)
    with tempfile.NamedTemporaryFile("w", suffix=".prototxt", delete=False) as f:
        f.write(text)
        path = f.name
    outs = []
    try:
        for sw in ({}, {"EPI_MAX": 0}):
            with dev_switches(**sw):
                net = Net(ctx, path)
                net.set_params(params)
                net.forward(torch.from_numpy(x).cuda())
                outs.append(net.output_numpy())
                net.close()
    finally:
        os.unlink(path)
    ref = torch_forward(graph, params, x)
    err = rel_l2(outs[0], ref)
    print("PReLU slopes in [-0.5, 1.5]: rel-L2 %.3e" % err)
    assert err < SMALL_TOL and ch_ok(outs[0], ref)
    np.testing.assert_array_equal(outs[0], outs[1])


# ---- split precision (opk_net_set_precision OPK_PRECISION_SPLIT) --------------------------------
# Every weight and activation an fp16 hi/lo pair, three MFMA passes per conv: the products are exact
# in fp32, so the result differs from the fp32 oracle only by fp32 summation order and the dropped
# x_lo * w_lo term (~2^-22 relative).  CPU emulation of the contract: rel-L2 6.3e-6
# for BODY_25 at 368x656 with full-strength heads.
SPLIT_TOL = 5e-5          # relative L2 of the net output
SPLIT_CHANNEL_TOL = 5e-4  # relative L2 of any single output channel


@pytest.mark.parametrize("n,h,w", [(2, 64, 96), (1, 368, 656)])
def test_body25_split_precision_vs_oracle(ctx, n, h, w):
    """BODY_25 in split precision against the fp32 oracle (three orders of magnitude closer than
    fp16), and back in fp16 precision the net gives a fresh fp16 net's output bit for bit."""
    from openpose_amd.api import PRECISION_FP16, PRECISION_SPLIT
    graph = body25.layers()
    params = synth.he_weights(graph, seed=23, out_scale=1.0)
    x = np.random.default_rng(24).uniform(-0.5, 0.5, (n, 3, h, w)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    net = Net(ctx, "builtin:BODY_25")
    net.set_params(params)
    net.forward(xd)
    fp16 = net.output_numpy()
    net.set_precision(PRECISION_SPLIT)
    with dev_switches(LAUNCH_LOG=1):
        net.forward(xd)
        kernels = {k for _, k in net.launch_log()}
    got = net.output_numpy()
    assert all("split" in k for k in kernels
               if k.startswith(("conv3_kernel", "conv3w8", "conv_image", "conv_head"))), kernels
    assert not any(k.startswith(("conv3w_", "conv1_fused")) for k in kernels), kernels
    ref = body25.forward(x, params, graph=graph)
    err, err16 = rel_l2(got, ref), rel_l2(fp16, ref)
    ch = channel_errors(got, ref)
    # against the exact (float64) forward, split precision is as close as the fp32 oracle itself:
    # both sit at fp32's reassociation noise (CPU, round 6: oracle 8.0e-6, torch fp32 2.5e-6)
    ex = torch_forward64(graph, params, x)
    err_ex, err_or = rel_l2(got, ex), rel_l2(ref, ex)
    print("BODY_25 %dx%dx%d split precision rel-L2 %.3e vs the fp32 oracle (fp16 %.3e), worst "
          "channel %.3e; vs float64: split %.3e, fp32 oracle %.3e"
          % (n, h, w, err, err16, ch.max(), err_ex, err_or))
    assert err < SPLIT_TOL and ch.max() < SPLIT_CHANNEL_TOL
    assert err < err16 / 20
    assert err_ex < 2 * err_or + 1e-6
    net.set_precision(PRECISION_FP16)
    net.forward(xd)
    np.testing.assert_array_equal(net.output_numpy(), fp16)


def test_split_precision_blobs_and_graphs(ctx):
    """Split precision on the other graph shapes the planner meets -- dense block + concat + 2x2 pool
    (pooled pairs), 7x7 CPM stages, 1x1 heads into a concat output -- against the fp32 oracle; and a
    named intermediate blob (caffe::Net::blob_by_name) reads back as hi + lo."""
    from openpose_amd.api import PRECISION_SPLIT
    x = np.random.default_rng(25).uniform(-0.5, 0.5, (2, 3, 64, 96)).astype(np.float32)
    for layers, seed in ((cpm_stage_graph(True), 5), (cpm_stage_graph(False), 6)):
        got, ref = run_graph(ctx, layers, x, seed=seed, precision=PRECISION_SPLIT)
        assert got.shape == ref.shape and rel_l2(got, ref) < SPLIT_TOL, rel_l2(got, ref)
    graph = body25.layers()
    params = synth.he_weights(graph, seed=26)
    net = Net(ctx, "builtin:BODY_25")
    net.set_params(params)
    net.set_precision(PRECISION_SPLIT)
    net.forward(torch.from_numpy(x).cuda())
    blob = net.blob("pool2_stage1")
    ref = body25.forward(x, params, graph=graph, stop_at="pool2_stage1")
    assert blob.shape == ref.shape and rel_l2(blob, ref) < SPLIT_TOL, rel_l2(blob, ref)


def test_split_precision_large_batch_frame_runs(ctx):
    """Split precision at a batch whose full-resolution layers exceed one conv3 launch's 24-bit
    position range (70 x 370 x 658 padded positions): the convs run in frame runs
    (conv3_runs), and every frame's output equals the same frame forwarded alone, bit for
    bit (an output's MFMA accumulation order does not depend on the batch)."""
    from openpose_amd.api import PRECISION_SPLIT
    n = 70
    net = Net(ctx, "builtin:BODY_25")
    net.set_params(synth.he_weights(net.convs(), seed=27))
    net.set_precision(PRECISION_SPLIT)
    x = np.random.default_rng(28).uniform(-0.5, 0.5, (n, 3, 368, 656)).astype(np.float32)
    net.forward(torch.from_numpy(x).cuda())
    got = net.output_numpy()
    for f in (0, n // 2, n - 1):
        net.forward(torch.from_numpy(x[f:f + 1]).cuda())
        np.testing.assert_array_equal(got[f], net.output_numpy()[0])


def test_split_precision_frame_runs_take_their_own_geometry(ctx):
    """a batch whose frame runs are smaller than the whole batch may put a run into
    another conv3 tile branch (another halo, so another strip count) than the planner chose for
    the batch.  At 96x96 the 64-channel full-resolution layer (conv1_2, split precision) holds 1,711
    frames per launch in 256-position tiles of two strips; 1,712 frames used to leave a 1-frame
    tail, whose 37 tiles take the 512-position branch (one strip), and the forward threw.  Runs are
    now even and each takes the geometry of its own frame count: every frame equals the frame
    alone, bit for bit."""
    from openpose_amd.api import PRECISION_SPLIT
    n = 1712
    net = Net(ctx, "builtin:BODY_25")
    net.set_params(synth.he_weights(net.convs(), seed=29))
    net.set_precision(PRECISION_SPLIT)
    x = np.random.default_rng(30).uniform(-0.5, 0.5, (n, 3, 96, 96)).astype(np.float32)
    with dev_switches(LAUNCH_LOG=1):
        net.forward(torch.from_numpy(x).cuda())
        runs = sum(1 for layer, _ in net.launch_log() if layer.split("+")[0] == "conv1_2")
    assert runs == 2, runs   # two even runs of 856 frames (conv1_2 + pool1 in one kernel)
    got = net.output_numpy()
    for f in (0, 855, 856, n - 1):
        net.forward(torch.from_numpy(x[f:f + 1]).cuda())
        np.testing.assert_array_equal(got[f], net.output_numpy()[0])
    net.close()


def test_split_pool_fusion_bit_identical(ctx):
    """Split precision with pool1 / pool2 / pool3 in conv3w8's epilogue (the pair of the larger hi + lo per
    window, the first in raster order on ties) equals the unfused conv + maxpool2_split_kernel bit
    for bit: the net output and the pooled blobs (8 frames at 368x656: enough tiles for the
    persistent geometry the fusion needs at both pooled layers)."""
    from openpose_amd.api import PRECISION_SPLIT
    x = np.random.default_rng(33).uniform(-0.5, 0.5, (8, 3, 368, 656)).astype(np.float32)
    params = synth.he_weights(body25.layers(), seed=34)
    outs = []
    for sw in ({}, {"POOL_FUSE": 0}):
        with dev_switches(LAUNCH_LOG=1, **sw):
            net = Net(ctx, "builtin:BODY_25")
            net.set_params(params)
            net.set_precision(PRECISION_SPLIT)
            net.forward(torch.from_numpy(x).cuda())
            fused = sum(1 for layer, _ in net.launch_log() if layer.endswith("+pool"))
            outs.append((fused, net.output_numpy(), net.blob("pool1_stage1"), net.blob("pool2_stage1"),
                         net.blob("pool3_stage1")))
            net.close()
    # conv1_2 + pool1 (conv3w8's 64-channel tile), conv2_2 + pool2, conv3_4 + pool3
    assert outs[0][0] == 3 and outs[1][0] == 0, (outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1:], outs[1][1:]):
        np.testing.assert_array_equal(a, b)
