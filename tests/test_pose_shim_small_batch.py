"""The pose drop-in with OPENPOSE_HIP_SMALL_BATCH (integration/openpose_hip_shim.cpp createNet): the
driver of tests/test_pose_shim.py with the variable set to 1 gives the heat maps, peaks and keypoints
of the C-ABI run (small-batch mode is bit-identical to the default planning, so the C-ABI net runs
it too); any value but 0 / 1 fails through op::error naming the variable."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests.test_pose_shim import BIN, _inputs, _read, _result


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(BIN), reason="driver not built (needs the reference headers)")
def test_pose_shim_small_batch_env(ctx):
    import torch
    from openpose_amd.api import Net, PoseExtractor

    with tempfile.TemporaryDirectory() as d:
        path, producer, scales, sizes, xs, field = _inputs(d)
        np.float32(2.0).tofile(os.path.join(d, "fns_scale.f32"))
        env = dict(os.environ, OPENPOSE_HIP_SMALL_BATCH="1")
        r = subprocess.run([BIN, d], capture_output=True, text=True, timeout=180, env=env)
        assert r.returncode == 0 and "pose driver ok" in r.stdout, r.stderr + r.stdout

        net = Net(ctx, "builtin:BODY_25", caffemodel=path)
        net.set_small_batch(True)
        dev = [torch.from_numpy(x).cuda() for x in xs]
        pose = PoseExtractor(ctx, net)
        pose.set_property(0, 0.06)
        pose.forward(dev[0], producer)
        kp, sc = pose.keypoints(0)
        gk, gs, _ = _result(d, "single")
        np.testing.assert_array_equal(gk, kp)
        np.testing.assert_array_equal(gs, sc)
        heat = pose.heatmaps_numpy()
        assert np.abs(heat).max() > 0
        np.testing.assert_array_equal(_read(d, "single_heat.f32").reshape(heat.shape[1:]), heat[0])
        np.testing.assert_array_equal(_read(d, "single_cand.f32").reshape(25, 128, 3),
                                      pose.peaks_numpy()[0])
        pose.forward_multi(dev, producer)   # the 4 scales: smaller nets, all on small tiles
        kp, sc = pose.keypoints(0)
        gk, gs, _ = _result(d, "multi")
        np.testing.assert_array_equal(gk, kp)
        np.testing.assert_array_equal(gs, sc)
        pose.close()
        net.forward(dev[0])
        np.testing.assert_array_equal(_read(d, "net_out0.f32"), net.output_numpy().ravel())
        net.close()

        # any value but 0 / 1 is refused, not defaulted (the net is created first: the error path
        # frees it)
        bad = dict(os.environ, OPENPOSE_HIP_SMALL_BATCH="yes")
        r = subprocess.run([BIN, d], capture_output=True, text=True, timeout=180, env=bad)
        assert r.returncode != 0 and "OPENPOSE_HIP_SMALL_BATCH must be 0 or 1" in r.stderr, \
            r.stderr + r.stdout
