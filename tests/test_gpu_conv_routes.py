"""The launches of every conv route, pinned: tests/golden/conv_route_traces.json holds, for each case of
tests/golden/make_conv_routes.CASES, every ``bg_*`` call that Conv2dFn / SubpixelConvFn / Deconv2dFn / ops.conv made
through ``functional.lib()`` in one forward and backward at the commit named in the file - before ``conv_route`` chose
the kernels in one place.  The same cases run here must make the same calls in the same order with the same
descriptors, flags and null pointers, and return tensors of the same types and shapes."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_conv_routes", os.path.join(HERE, "golden", "make_conv_routes.py"))
make_conv_routes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_conv_routes)
CASES = make_conv_routes.CASES

with open(os.path.join(HERE, "golden", "conv_route_traces.json")) as _fh:
    GOLDEN = json.load(_fh)


def test_table_and_golden_file_hold_the_same_cases():
    assert len(GOLDEN["commit"]) == 40
    assert sorted(GOLDEN["cases"]) == sorted(CASES)
    for name, c in CASES.items():
        assert GOLDEN["cases"][name]["case"] == c, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_route_makes_the_recorded_calls(name):
    want = GOLDEN["cases"][name]
    got = json.loads(json.dumps(make_conv_routes.trace(name, CASES[name])))
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, "call %d" % i
    assert got["outputs"] == want["outputs"]
    assert got["y_is_accumulator"] == want["y_is_accumulator"]
