"""Every kernel route of the launchers around the net (input.hip, paf.hip, nms.hip) and the test
case that must reach it.

A route is a name the launcher writes into the launch log (note_launch, literal in the source).
The GPU case named here asserts with ran() that its route is in the log of its own launches;
tests/test_kernel_routes.py (CPU) asserts that the names in the source are exactly the keys of
ROUTES, so a new route without a case fails before any GPU runs.
"""
import os
import re

KERNELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "openpose_amd", "csrc",
                       "kernels")
FILES = ("input.hip", "paf.hip", "nms.hip")

_WARP = "tests.test_gpu_warp_routes"
_PAF = "tests.test_gpu_paf_scores"
_PIPE = "tests.test_gpu_pipeline"
# route: (module, test function) of the case that asserts it ran
ROUTES = {
    "cvmat_to_input_lds<2,a16>": (_WARP, "test_lds_boundary_widths"),
    "cvmat_to_input_lds<2>": (_WARP, "test_padded_rows_and_misaligned_base"),
    "cvmat_to_input_lds<4,a16>": (_WARP, "test_lds_boundary_widths"),
    "cvmat_to_input_lds<4>": (_WARP, "test_odd_width_upscaled"),
    "cvmat_to_input<2>": (_WARP, "test_direct_kernels"),
    "cvmat_to_input<4>": (_WARP, "test_direct_kernels"),
    "paf_dense<lds,spl>": (_PAF, "test_scores_every_route"),
    "paf_dense<lds>": (_PAF, "test_scores_every_route"),
    "paf_dense<spl>": (_PAF, "test_scores_every_route"),
    "paf_dense": (_PAF, "test_scores_every_route"),
    "paf_compact<lds,spl>": (_PAF, "test_scores_every_route"),
    "paf_compact<lds>": (_PAF, "test_scores_every_route"),
    "paf_compact<spl>": (_PAF, "test_scores_every_route"),
    "paf_compact": (_PAF, "test_scores_every_route"),
    "nms_detect": ("tests.test_gpu_postprocess", "test_nms_materialised_route"),
    "nms_detect_walk2<1,cold>": (_PIPE, "test_nms_walk_variants_bitexact"),
    "nms_detect_walk2<1>": (_PIPE, "test_nms_cold_windows_bitexact"),
    "nms_detect_walk2<2>": (_PIPE, "test_multiscale_other_scale_numbers_bitexact"),
    "nms_detect_walk2<3>": (_PIPE, "test_multiscale_other_scale_numbers_bitexact"),
    "nms_detect_walk2<4>": (_PIPE, "test_nms_walk_variants_bitexact"),
    "nms_detect_stream<1>": (_PIPE, "test_nms_walk_variants_bitexact"),
    "nms_detect_stream<2>": (_PIPE, "test_nms_ring_walk_two_three_sources"),
    "nms_detect_stream<3>": (_PIPE, "test_nms_ring_walk_two_three_sources"),
    "nms_detect_stream<4>": (_PIPE, "test_nms_walk_variants_bitexact"),
    "nms_detect_lazy": (_PIPE, "test_multiscale_other_scale_numbers_bitexact"),
}


def source_routes(text):
    """The string literals inside the note_launch(...) calls of a source text."""
    names = []
    for m in re.finditer(r"\bnote_launch\(", text):
        call = text[m.end():text.index(";", m.end())]
        names += re.findall(r'"([^"]*)"', call)
    return names


def routes_in_source():
    out = {}
    for f in FILES:
        with open(os.path.join(KERNELS, f)) as fh:
            out[f] = source_routes(fh.read())
    return out


def ran(log, route):
    """Assert that `route` is a known route and that a launch of it is in the launch log."""
    assert route in ROUTES, "unknown route %s" % route
    kernels = [k for _, k in log]
    assert route in kernels, "%s did not run: %s" % (route, kernels)
