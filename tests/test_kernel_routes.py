"""The route names in the launchers' source are exactly the routes that have a test case
(tests/kernel_routes.py): a launcher that gains a route fails here, without a GPU, until a case
reaches it."""
import os
import re

from tests import kernel_routes as kr


def test_every_route_in_the_source_has_a_case():
    found = kr.routes_in_source()
    names = [n for f in kr.FILES for n in found[f]]
    assert all(found[f] for f in kr.FILES)
    assert not [n for n in names if "%" in n], "route names are literal, not formatted"
    assert len(names) == len(set(names)), "a route name is noted twice"
    assert set(names) == set(kr.ROUTES), (sorted(set(names) - set(kr.ROUTES)),
                                          sorted(set(kr.ROUTES) - set(names)))
    assert len(found["input.hip"]) == 6 and len(found["paf.hip"]) == 8


def test_every_launch_is_noted():
    """No launch of these files goes unnamed: as many notes as launch sites (the NMS stream macro
    holds three launches for the names of each of its four uses; nms_finalize runs after every
    route and is not one)."""
    for f in kr.FILES:
        with open(os.path.join(kr.KERNELS, f)) as fh:
            text = fh.read()
        launches = len(re.findall(r"hipLaunchKernelGGL\(", text))
        notes = len(re.findall(r"\bnote_launch\(", text))
        if f == "nms.hip":
            assert (launches, notes) == (6, 6)   # detect, 3 in the macro, lazy, finalize
        elif f == "input.hip":
            assert (launches, notes) == (3, 6)   # the LDS macro holds one launch for four names
        else:
            assert launches == notes == 8


def test_every_case_exists_and_asserts_its_route():
    here = os.path.dirname(os.path.abspath(__file__))
    for route, (module, func) in kr.ROUTES.items():
        with open(os.path.join(here, module.split(".")[-1] + ".py")) as fh:
            text = fh.read()
        m = re.search(r"^def %s\(.*?(?=^def |\Z)" % re.escape(func), text, re.S | re.M)
        assert m, "%s: no %s in %s" % (route, func, module)
        # the case asserts its route itself or through the module's launch helper
        assert re.search(r"\b(ran|_launch|_run)\(", m.group(0)), \
            "%s: %s does not assert a route" % (route, func)
        assert "ran(" in text


def test_launch_log_attaches_and_detaches_on_the_host():
    """opk_launch_log_begin / _end need no device: a block without launches gives an empty list,
    and the lines stay readable until the next begin."""
    from openpose_amd import _lib
    from openpose_amd.api import launch_log
    with launch_log() as log:
        pass
    assert log == []
    import ctypes
    need = ctypes.c_size_t()
    assert _lib.load().opk_launch_log_end(None, 0, ctypes.byref(need)) == 0 and need.value == 1
    assert _lib.load().opk_launch_log_end(None, 0, None) != 0
