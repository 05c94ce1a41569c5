"""The restatement of the 3-D reconstruction text (tests/triangulate_cases.py) against an
independent implementation of its one restated step: the same flow with the null vector from
LAPACK's SVD (numpy.linalg.svd).  CPU only, no library."""
import numpy as np
import pytest

from tests import triangulate_cases as tc

NOISES = (0.0, 0.5, 3.0, 15.0)
RIGS_PER_CASE = 3
STEPS, PARTS = 2, 6


def _seed(V, noise, r):
    return 7000 + 1000 * V + 10 * int(noise * 10) + r


@pytest.fixture(scope="module")
def runs():
    """Every seeded rig once, through both variants: [(V, noise, jacobi, jacobi info, lapack,
    lapack info)]."""
    out = []
    for V in range(2, 8):
        for noise in NOISES:
            for r in range(RIGS_PER_CASE):
                rng = np.random.default_rng(_seed(V, noise, r))
                P, sizes = tc.ring_rig(rng, V)
                kp, _ = tc.scene(rng, P, STEPS, PARTS, noise)
                ji, li = {}, {}
                j = tc.reconstruct(P, sizes, -1, kp, info=ji)
                l = tc.reconstruct(P, sizes, -1, kp, null=tc.lapack_null, info=li)
                out.append((V, noise, j, ji, l, li))
    return out


def test_jacobi_converges_before_the_sweep_limit(runs):
    # the 30-sweep cap is never the exit on these inputs
    for V, noise, _, ji, _, _ in runs:
        assert ji["unconverged"] == 0 and ji["max_sweeps"] < 30, (V, noise, ji["max_sweeps"])


def test_points_agree_with_lapack_in_fp64(runs):
    # 1e-12 relative: five orders below a float32 ulp (6e-8), which is what lets a float that
    # differs be read as a rounding boundary.  Both null vectors are off by a small multiple of
    # eps = 2.2e-16 times the conditioning of these rigs (cameras 3.5-5.5 m from points within
    # 0.35 m), of the order of 1e2-1e3.
    worst = 0.0
    for V, noise, _, ji, _, li in runs:
        assert ji["x64"].keys() == li["x64"].keys()
        for key, a in ji["x64"].items():
            a, b = np.array(a), np.array(li["x64"][key])
            worst = max(worst, float(np.linalg.norm(a - b) / np.linalg.norm(b)))
    print("largest relative fp64 difference: %.3g" % worst)
    assert worst < 1e-12


def test_floats_within_one_ulp_and_decisions_equal(runs):
    left_out, cases = 0, 0
    for V, noise, j, _, l, li in runs:
        cases += 1
        if li.get("near", 0):   # the LAPACK error sits on a threshold: either decision is right
            left_out += 1
            continue
        assert np.array_equal(j[1], l[1]), (V, noise, "status")
        assert np.array_equal(j[2] >= 0, l[2] >= 0), (V, noise, "attempted")
        assert np.array_equal(j[3], l[3]), (V, noise, "dropped view")
        assert np.array_equal(j[0][..., 3], l[0][..., 3]), (V, noise, "accepted")
        # a float that differs sits on a rounding boundary (the fp64 points agree to 1e-12)
        assert tc.ulp_apart(j[0], l[0]) <= 1.0, (V, noise)
        # the errors to the same 1e-12; a point off by 1e-12 relative moves its projections, of
        # the order of 1e3 px, by 1e-9 px, which is the floor for errors near zero
        assert np.allclose(j[2], l[2], rtol=1e-12, atol=1e-9, equal_nan=True), (V, noise)
    # the seeds are chosen so that the LAPACK variant alone leaves out none
    assert left_out == 0 and left_out <= 0.01 * cases


def test_cases_reach_every_branch(runs):
    dropped = sum(int((j[3] >= 0).sum()) for _, _, j, _, _, _ in runs)
    undropped_4 = sum(int((j[3] < 0).sum()) for V, _, j, _, _, _ in runs if V >= 4)
    rejected = sum(int(((j[2] >= 0) & (j[0][..., 3] == 0)).sum()) for _, _, j, _, _, _ in runs)
    accepted = sum(int(j[0][..., 3].sum()) for _, _, j, _, _, _ in runs)
    assert dropped > 0 and undropped_4 > 0 and rejected > 0 and accepted > 0


def test_camera_matrix_is_the_sequential_product():
    rng = np.random.default_rng(5)
    K, Rt = rng.normal(size=(3, 3)), rng.normal(size=(3, 4))
    assert np.allclose(tc.camera_matrix(K, Rt), K @ Rt, rtol=1e-13, atol=1e-15)
