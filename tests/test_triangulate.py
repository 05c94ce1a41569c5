"""CPU: opk_triangulate_host (host/triangulate.cpp over kernels/triangulate_dev.h) bit for bit
against the numpy restatement of the include/opk.h text (tests/triangulate_cases.py) -- xyz, status,
errors and dropped views -- on the smallest cases that reach each branch; the argument checks;
opk_camera_matrix; the 3-D arrays in the people JSON; and the same host code under
AddressSanitizer / UBSan in a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

from openpose_amd import api
from openpose_amd import build as opk_build
from tests import triangulate_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZE = (1280, 720)
MAX_ACC = tc.max_acceptable([SIZE])   # 20.96 px


def both(P, sizes, kp, present=None, min_views=-1):
    """The library's host route, checked bit for bit against the restatement."""
    got = api.Triangulator(P, sizes, min_views).reconstruct(kp, present)
    want = tc.reconstruct(P, sizes, min_views, kp, present)
    for g, w, what in zip(got, want, ("xyz", "status", "errors", "dropped")):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert np.array_equal(g, w, equal_nan=(what == "errors")), what
    return got


def rig_and_scene(seed, V, steps=1, parts=1, noise=0.0):
    rng = np.random.default_rng(seed)
    P, sizes = tc.ring_rig(rng, V, SIZE)
    kp, pts = tc.scene(rng, P, steps, parts, noise)
    return P, sizes, kp, pts


def case_two_views_one_point(run):
    P, sizes, kp, pts = rig_and_scene(1, 2)
    xyz, status, errors, dropped = run(P, sizes, kp)
    assert status[0] == 1 and xyz[0, 0, 3] == 1 and dropped[0, 0] == -1
    np.testing.assert_allclose(xyz[0, 0, :3], pts[0, 0], atol=1e-3)   # float32 pixels in


def test_two_views_one_point():
    case_two_views_one_point(both)


def case_seven_views(run):
    P, sizes, kp, pts = rig_and_scene(2, 7, steps=2, parts=4, noise=1.0)
    xyz, status, _, _ = run(P, sizes, kp)
    assert status.tolist() == [1, 1] and xyz[..., 3].all()
    np.testing.assert_allclose(xyz[..., :3], pts, atol=0.02)


def test_seven_views():
    case_seven_views(both)


def case_array_sizes(run, parts):
    P, sizes, kp, _ = rig_and_scene(10 + parts, 4, steps=2, parts=parts, noise=2.0)
    kp[0, 1, ::3, 2] = 0.1     # some parts unseen by one view, some by two
    kp[0, 2, ::6, 2] = 0.1
    xyz, status, errors, _ = run(P, sizes, kp)
    assert status.tolist() == [1, 1]
    assert (errors[0, ::6] == -1).all() and (errors[0, 1::3] >= 0).all()


@pytest.mark.parametrize("parts", [25, 70, 21])
def test_array_sizes(parts):
    case_array_sizes(both, parts)


def case_fewer_than_two_present_views_is_not_a_3d_problem(run):
    P, sizes, kp, _ = rig_and_scene(3, 3, steps=3, parts=2)
    present = np.array([[0, 0, 0], [0, 1, 0], [1, 0, 1]], np.int32)
    xyz, status, errors, _ = run(P, sizes, kp, present, min_views=2)
    assert status.tolist() == [0, 0, 1]
    assert not xyz[:2].any() and (errors[:2] == -1).all() and xyz[2, :, 3].all()


def test_fewer_than_two_present_views_is_not_a_3d_problem():
    case_fewer_than_two_present_views_is_not_a_3d_problem(both)


def case_part_seen_by_too_few_views_is_not_attempted(run):
    P, sizes, kp, _ = rig_and_scene(4, 4, parts=3)       # effective min_views 3
    kp[0, 0, 1, 2] = kp[0, 3, 1, 2] = 0.0               # part 1: two valid views
    xyz, status, errors, dropped = run(P, sizes, kp)
    assert status[0] == 1 and errors[0, 1] == -1 and not xyz[0, 1].any()
    assert xyz[0, 0, 3] == 1 and xyz[0, 2, 3] == 1


def test_part_seen_by_too_few_views_is_not_attempted():
    case_part_seen_by_too_few_views_is_not_attempted(both)


def case_no_attempted_part_is_status_0(run):
    P, sizes, kp, _ = rig_and_scene(5, 3, parts=4)
    kp[..., 2] = 0.2
    xyz, status, errors, _ = run(P, sizes, kp)
    assert status[0] == 0 and not xyz.any() and (errors == -1).all()


def test_no_attempted_part_is_status_0():
    case_no_attempted_part_is_status_0(both)


def case_score_threshold_is_strict(run):
    P, sizes, kp, _ = rig_and_scene(6, 2)
    kp[0, 0, 0, 2] = np.float32(0.35)
    _, status, errors, _ = run(P, sizes, kp)
    assert status[0] == 0 and errors[0, 0] == -1
    kp[0, 0, 0, 2] = np.nextafter(np.float32(0.35), np.float32(1))
    _, status, errors, _ = run(P, sizes, kp)
    assert status[0] == 1 and errors[0, 0] >= 0


def test_score_threshold_is_strict():
    case_score_threshold_is_strict(both)


def case_border_is_strict(run, axis, edge):
    P, sizes, kp, _ = rig_and_scene(7, 2)
    inward = np.float32(640 if axis == 0 else 360)
    kp[0, 1, 0, axis] = np.float32(edge)
    _, status, errors, _ = run(P, sizes, kp)
    assert status[0] == 0 and errors[0, 0] == -1
    kp[0, 1, 0, axis] = np.nextafter(np.float32(edge), inward)
    _, status, errors, _ = run(P, sizes, kp)
    assert status[0] == 1 and errors[0, 0] >= 0
    for bad in (np.nan, np.inf, -np.inf):            # never get in
        kp[0, 1, 0, axis] = bad
        _, status, _, _ = run(P, sizes, kp)
        assert status[0] == 0


@pytest.mark.parametrize("axis, edge", [(0, 8), (0, SIZE[0] - 8), (1, 8), (1, SIZE[1] - 8)])
def test_border_is_strict(axis, edge):
    case_border_is_strict(both, axis, edge)


def case_outlier_view_of_four_is_dropped(run, view):
    P, sizes, kp, pts = rig_and_scene(8, 4, parts=2, noise=0.3)
    kp[0, view, 0, 0] += 80
    xyz, _, errors, dropped = run(P, sizes, kp)
    assert dropped[0].tolist() == [view, -1]
    assert xyz[0, :, 3].all() and errors[0, 0] < 2
    np.testing.assert_allclose(xyz[0, :, :3], pts[0], atol=0.01)


@pytest.mark.parametrize("view", range(4))
def test_outlier_view_of_four_is_dropped(view):
    case_outlier_view_of_four_is_dropped(both, view)


def case_four_consistent_views_drop_none(run):
    P, sizes, kp, _ = rig_and_scene(9, 4, parts=3, noise=0.5)
    xyz, _, _, dropped = run(P, sizes, kp)
    assert (dropped == -1).all() and xyz[..., 3].all()


def test_four_consistent_views_drop_none():
    case_four_consistent_views_drop_none(both)


def twin_case():
    """Seven views, views 0 and 1 the same camera with the same detection, 150 px off: the sets
    without 0 and without 1 hold the same rows, so their errors are equal to the bit."""
    rng = np.random.default_rng(17)
    P, sizes = tc.ring_rig(rng, 7, SIZE)
    P[1] = P[0]
    kp, _ = tc.scene(rng, P, 1, 2, 0.3)
    kp[0, 1] = kp[0, 0]
    kp[0, :2, 0, 0] += 150
    return P, sizes, kp


def case_equal_subsets_keep_the_first(run):
    P, sizes, kp = twin_case()
    Pl = [[[float(e) for e in row] for row in m] for m in P]
    xs, ys = [float(v) for v in kp[0, :, 0, 0]], [float(v) for v in kp[0, :, 0, 1]]
    subsets = [tc.solve(Pl, xs, ys, [v for v in range(7) if v != i])[1] for i in range(7)]
    assert subsets[0] == subsets[1] == min(subsets)      # the case is the tie it claims to be
    _, _, _, dropped = run(P, sizes, kp)
    assert dropped[0].tolist() == [0, -1]


def test_equal_subsets_keep_the_first():
    case_equal_subsets_keep_the_first(both)


def between_case():
    """Seven views, 14 px noise in each; part 5 sits badly (15.8 px) but no subset is below 0.9 e."""
    rng = np.random.default_rng(22)
    P, sizes = tc.ring_rig(rng, 7, SIZE)
    kp, _ = tc.scene(rng, P, 1, 6, 14.0)
    return P, sizes, kp


def case_subset_that_is_not_considerably_better_is_not_taken(run):
    P, sizes, kp = between_case()
    Pl = [[[float(e) for e in row] for row in m] for m in P]
    xs, ys = [float(v) for v in kp[0, :, 5, 0]], [float(v) for v in kp[0, :, 5, 1]]
    e = tc.solve(Pl, xs, ys, list(range(7)))[1]
    best = min(tc.solve(Pl, xs, ys, [v for v in range(7) if v != i])[1] for i in range(7))
    assert e > 0.5 * MAX_ACC and 0.9 * e <= best < e      # better, but not considerably
    _, _, errors, dropped = run(P, sizes, kp)
    assert dropped[0, 5] == -1 and errors[0, 5] == e
    assert (dropped[0, :5] >= 0).any()                    # others of the array do drop a view


def test_subset_that_is_not_considerably_better_is_not_taken():
    case_subset_that_is_not_considerably_better_is_not_taken(both)


def case_three_views_have_no_leave_one_out(run):
    P, sizes, kp, _ = rig_and_scene(10, 3, parts=2, noise=0.3)
    kp[0, 1, 0, 0] += 200
    xyz, status, errors, dropped = run(P, sizes, kp, min_views=2)
    assert dropped[0, 0] == -1 and errors[0, 0] >= MAX_ACC          # rejected by maxAcc
    assert status[0] == 1 and not xyz[0, 0].any() and xyz[0, 1, 3] == 1


def test_three_views_have_no_leave_one_out():
    case_three_views_have_no_leave_one_out(both)


def case_part_far_worse_than_the_rest_is_rejected(run):
    P, sizes, kp, _ = rig_and_scene(11, 3, parts=12, noise=0.3)
    kp[0, 2, 5, 1] += 30
    xyz, _, errors, _ = run(P, sizes, kp)
    total = errors[0].sum() / 12
    assert 5 * total <= errors[0, 5] < MAX_ACC                      # rejected by 5*total alone
    assert not xyz[0, 5].any() and np.delete(xyz[0, :, 3], 5).all()


def test_part_far_worse_than_the_rest_is_rejected():
    case_part_far_worse_than_the_rest_is_rejected(both)


def case_identical_cameras_follow_the_text_and_a_nan_clears_the_array(run):
    rng = np.random.default_rng(12)
    P, sizes = tc.ring_rig(rng, 3, SIZE)
    K = np.array([[1000., 0, 640], [0, 1000., 360], [0, 0, 1]])
    P[0] = P[1] = tc.camera_matrix(K, np.eye(3, 4))                 # twice the camera at the origin
    kp = np.zeros((1, 3, 2, 3), np.float32)
    kp[0, :, :, 2] = 0.9
    kp[0, :, 0, :2] = (700, 300)
    kp[0, :, 1, :2] = (500, 400)
    kp[0, 2, 0, 2] = 0.0        # part 0: the identical pair only -- a rank-deficient A
    xyz, status, errors, _ = run(P, sizes, kp, min_views=2)
    assert np.isnan(errors[0, 0]) and np.isfinite(errors[0, 1])
    assert status[0] == 1 and not xyz.any()                         # total is NaN: nothing accepted
    kp[0, 1, 0, 2] = 0.0        # part 0 no longer attempted: part 1 decides alone
    xyz, status, errors, _ = run(P, sizes, kp, min_views=2)
    assert errors[0, 0] == -1 and status[0] == 1


def test_identical_cameras_follow_the_text_and_a_nan_clears_the_array():
    case_identical_cameras_follow_the_text_and_a_nan_clears_the_array(both)


def case_min_views(run, min_views, attempted):
    P, sizes, kp, _ = rig_and_scene(13, 5, parts=2)
    kp[0, 2:, 0, 2] = 0.0                                           # part 0: views 0 and 1
    _, status, errors, _ = run(P, sizes, kp, min_views=min_views)
    assert (errors[0, 0] >= 0) == attempted and errors[0, 1] >= 0 and status[0] == 1


@pytest.mark.parametrize("min_views, attempted", [(2, True), (3, False), (-1, False)])
def test_min_views(min_views, attempted):
    case_min_views(both, min_views, attempted)


# every case above as (id, function, arguments): tests/test_gpu_triangulate.py runs them, their
# assertions included, through the kernels as well
CASES = [
    ("two_views_one_point", case_two_views_one_point, ()),
    ("seven_views", case_seven_views, ()),
    ("fewer_than_two_present_views", case_fewer_than_two_present_views_is_not_a_3d_problem, ()),
    ("too_few_views", case_part_seen_by_too_few_views_is_not_attempted, ()),
    ("no_attempted_part", case_no_attempted_part_is_status_0, ()),
    ("score_threshold", case_score_threshold_is_strict, ()),
    ("four_consistent_views", case_four_consistent_views_drop_none, ()),
    ("equal_subsets", case_equal_subsets_keep_the_first, ()),
    ("subset_not_considerably_better", case_subset_that_is_not_considerably_better_is_not_taken, ()),
    ("three_views_outlier_max_acc", case_three_views_have_no_leave_one_out, ()),
    ("far_worse_than_the_rest", case_part_far_worse_than_the_rest_is_rejected, ()),
    ("identical_cameras_nan", case_identical_cameras_follow_the_text_and_a_nan_clears_the_array, ()),
]
CASES += [("array_sizes-%d" % p, case_array_sizes, (p,)) for p in (25, 70, 21)]
CASES += [("border-%d-%d" % ae, case_border_is_strict, ae)
          for ae in ((0, 8), (0, SIZE[0] - 8), (1, 8), (1, SIZE[1] - 8))]
CASES += [("outlier_view-%d" % v, case_outlier_view_of_four_is_dropped, (v,)) for v in range(4)]
CASES += [("min_views-%d" % mv, case_min_views, (mv, att))
          for mv, att in ((2, True), (3, False), (-1, False))]


def test_argument_errors():
    rng = np.random.default_rng(14)
    P, sizes = tc.ring_rig(rng, 7, SIZE)
    P8, sizes8 = np.concatenate([P, P[:1]]), np.concatenate([sizes, sizes[:1]])
    for args in ((P[:1], sizes[:1]), (P8, sizes8), (P, sizes, 0), (P, sizes, 1)):
        with pytest.raises(api.OpkError, match="opk error 1"):
            api.Triangulator(*args)
    bad = P.copy()
    bad[3, 1, 2] = np.nan
    with pytest.raises(api.OpkError, match="opk error 1"):
        api.Triangulator(bad, sizes)
    api.Triangulator(P, sizes, 2)
    api.Triangulator(P[:2], sizes[:2], -5)


def test_camera_matrix():
    rng = np.random.default_rng(15)
    K = np.array([[1234.5, 0.3, 641.2], [0, 1230.1, 355.7], [0, 0, 1]])
    Rt = rng.normal(size=(3, 4))
    got = api.camera_matrix(K, Rt)
    assert np.array_equal(got, tc.camera_matrix(K, Rt))
    np.testing.assert_allclose(got, K @ Rt, rtol=1e-13)


# ---- the 3-D arrays in the people JSON -----------------------------------------------------------
def test_people_json_with_3d_arrays():
    """tests/golden/people_3d.json is written by hand from savePeopleJson (fileStream.cpp:306-344):
    each array's row of the person, [parts][4] values for the 3-D ones."""
    kp = np.array([[[1.5, 2.0, 0.25], [0.0, 0.0, 0.0]]], np.float32)
    body3 = np.array([[[0.5, -1.25, 3.0, 1.0], [0.0, 0.0, 0.0, 0.0]]], np.float32)
    left3 = np.array([[[0.125, 2.0, 4.0, 1.0]]], np.float32)
    vec = api.datum_keypoint_vector(kp, pose_keypoints_3d=body3,
                                    hand_keypoints_3d=(left3, np.zeros((0, 1, 4), np.float32)))
    with open(os.path.join(GOLDEN, "people_3d.json")) as f:
        assert api.people_json(vec) == f.read().rstrip("\n")


def test_datum_keypoint_vector_without_3d_is_unchanged():
    kp = np.array([[[1.5, 2.0, 0.25], [0.0, 0.0, 0.0]]], np.float32)
    text = api.people_json(api.datum_keypoint_vector(kp))
    assert text == ('{"version":1.3,"people":[{"person_id":[-1],"pose_keypoints_2d":[1.5,2,0.25,0,0,0],'
                    '"face_keypoints_2d":[],"hand_left_keypoints_2d":[],"hand_right_keypoints_2d":[],'
                    '"pose_keypoints_3d":[],"face_keypoints_3d":[],"hand_left_keypoints_3d":[],'
                    '"hand_right_keypoints_3d":[]}]}')
    vec = api.datum_keypoint_vector(kp)
    assert [name for _, name in vec][5:] == ["pose_keypoints_3d", "face_keypoints_3d",
                                             "hand_left_keypoints_3d", "hand_right_keypoints_3d"]
    assert all(a is None for a, _ in vec[5:])


# ---- the host code under AddressSanitizer / UBSan, as a plain program ----------------------------
def _host_compiler():
    llvm = os.path.join(os.path.dirname(os.path.realpath(opk_build.HIPCC)), "..", "lib", "llvm")
    return os.path.join(llvm, "bin", "clang++"), os.path.join(
        os.path.dirname(os.path.realpath(opk_build.HIPCC)), "..", "include")


def test_host_route_under_sanitizers(tmp_path):
    cxx, hip_include = _host_compiler()
    if not os.path.exists(cxx):
        pytest.skip("no host compiler beside hipcc")
    exe = str(tmp_path / "triangulate_driver")
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-D__HIP_PLATFORM_AMD__", "-I" + hip_include, "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "triangulate_driver.cpp"),
           os.path.join(ROOT, "openpose_amd", "csrc", "host", "triangulate.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "libclang_rt" in r.stderr:
        pytest.skip("sanitizer runtime missing")
    assert r.returncode == 0, r.stderr
    # the outlier case (leave-one-out runs), 70 parts, an absent view, a short-sighted part
    P, sizes, kp, _ = rig_and_scene(16, 5, steps=2, parts=70, noise=1.0)
    kp[0, 1, ::2, 0] += 60
    kp[1, 3, 5, 2] = 0.0
    present = np.array([[1, 1, 1, 1, 1], [1, 0, 1, 1, 1]], np.int32)
    want = both(P, sizes, kp, present)
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(src, "wb") as f:
        f.write(np.array([5, -1, 2, 70], np.int32).tobytes() + P.tobytes()
                + np.ascontiguousarray(sizes, np.int32).tobytes() + kp.tobytes() + present.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "triangulate ok" in r.stdout, r.stdout + r.stderr
    raw = open(dst, "rb").read()
    at = 0
    for w in want:
        got = np.frombuffer(raw, w.dtype, w.size, at).reshape(w.shape)
        at += w.nbytes
        assert np.array_equal(got, w, equal_nan=True)
    assert at == len(raw)
