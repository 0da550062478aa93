"""treedetection_amd.crown_device, the base layer of the crown stage's device wrappers, on the CPU: the packed-ring helpers on a
crafted ring set, the stand-in for an empty array, the declined-path line, and the layering of the crown-stage modules, read from
their sources with ``ast`` (importing one of them imports the whole package)."""
import ast
import os

import numpy as np
import pytest

from treedetection_amd import crown_device as CD

NAN = float("nan")
RINGS = [
    np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 3.0], [0.0, 3.0], [0.0, 0.0]]),             # closed
    np.array([[10.5, -2.0], [12.0, -2.0], [11.0, 7.25]]),                               # open
    np.zeros((0, 2)),                                                                   # no vertices
    np.array([[1.0, 1.0], [NAN, 2.0], [3.0, 5.0], [0.5, 4.0]]),                         # a NaN x
    np.array([[412000.0, 5318000.0], [412004.0, 5318000.5], [412002.0, 5318009.0], [412000.0, 5318000.0]]),     # closed, map units
]
XY, START = CD.pack_rings(RINGS)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_crafted_set_packs_as_expected():
    assert START.tolist() == [0, 4, 7, 7, 11, 14] and XY.shape == (14, 2)


@pytest.mark.parametrize("idx", [[], [0, 1, 2, 3, 4], [4, 2, 0, 3, 1], [1, 1, 3, 1, 0, 0], [2], [2, 2], [3]])
def test_take_rings_is_pack_rings_of_the_selection(idx):
    sub_xy, sub_start = CD.take_rings(XY, START, np.array(idx, dtype=np.int64))
    want_xy, want_start = CD.pack_rings([RINGS[i] for i in idx])
    assert same_bits(sub_xy, want_xy) and same_bits(sub_start, want_start)
    assert sub_xy.dtype == np.float64 and sub_start.dtype == np.int64
    assert sub_xy.flags.c_contiguous and sub_start.flags.c_contiguous
    assert sub_xy.ndim == 2 and sub_xy.shape[1] == 2 and sub_start.shape == (len(idx) + 1,)
    assert sub_start[0] == 0 and sub_start[-1] == len(sub_xy)


def test_take_rings_takes_a_list_and_leaves_its_input_alone():
    xy, start = XY.copy(), START.copy()
    sub_xy, _ = CD.take_rings(xy, start, [4, 0])
    assert same_bits(xy, XY) and same_bits(start, START) and not np.shares_memory(sub_xy, xy)


def test_packed_boxes():
    boxes = CD.packed_boxes(XY, START)
    assert boxes.dtype == np.float64 and boxes.shape == (5, 4)
    assert boxes[0].tolist() == [0.0, 0.0, 4.0, 3.0]
    assert boxes[1].tolist() == [10.5, -2.0, 12.0, 7.25]
    assert np.isnan(boxes[2]).all()                                                     # no vertices: pairs with nothing
    assert np.isnan(boxes[3, [0, 2]]).all() and boxes[3, [1, 3]].tolist() == [1.0, 5.0]  # the NaN x reaches both x bounds
    assert boxes[4].tolist() == [412000.0, 5318000.0, 412004.0, 5318009.0]
    assert same_bits(CD.ring_boxes(RINGS), boxes)


def test_nonempty():
    for a in (XY, START, np.zeros(3, np.int32), np.ones((1, 2))):
        assert CD.nonempty(a) is a
    for empty in (np.zeros((0, 2)), np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint32)):
        got = CD.nonempty(empty)
        assert got.shape == (1,) + empty.shape[1:] and got.dtype == empty.dtype and not got.any() and got.flags.c_contiguous


def test_decline_prints_one_line(capsys):
    assert CD.decline("x", "y") is None
    assert capsys.readouterr().out == "x: y: using the host function\n"


# ---- layering ---------------------------------------------------------------------------------------------------------------------
PACKAGE = os.path.dirname(os.path.abspath(CD.__file__))
LOWER = ("crown_device", "box_pairs", "crown_rasters", "cleaning", "evaluation", "vector")


def imports_of(module, module_level_only=False):
    """(sibling names, other top-level module names) that the source of treedetection_amd/<module>.py imports."""
    with open(os.path.join(PACKAGE, module + ".py")) as f:
        tree = ast.parse(f.read())
    siblings, others = set(), set()

    def split(name, level):
        """A dotted name as (parts below the package, is it inside the package)."""
        parts = name.split(".") if name else []
        if level == 0 and parts[:1] == ["treedetection_amd"]:
            return parts[1:], True
        return parts, level > 0

    def visit(node):
        for child in ast.iter_child_nodes(node):
            if module_level_only and isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda, ast.ClassDef)):
                continue
            if isinstance(child, ast.Import):
                for alias in child.names:
                    parts, inside = split(alias.name, 0)
                    (siblings if inside else others).update(parts[:1])
            elif isinstance(child, ast.ImportFrom):
                parts, inside = split(child.module, child.level)
                if not inside:
                    others.add(parts[0])
                else:                           # ``from .x import y`` names x; ``from . import y`` names y
                    siblings.update(parts[:1] or [alias.name for alias in child.names])
            visit(child)

    visit(tree)
    return siblings, others


def test_the_reader_sees_the_imports_of_a_module_it_knows():
    siblings, others = imports_of("postprocessing")
    assert {"_lib", "box_pairs", "cleaning", "crown_device", "crown_rasters", "geotiff", "gpkg", "stitching"} <= siblings
    assert {"numpy", "torch", "yaml"} <= others
    assert "torch" in imports_of("box_pairs")[1] and "validity" in imports_of("cleaning")[0]      # function-level imports are seen


@pytest.mark.parametrize("module", LOWER)
def test_nothing_below_postprocessing_imports_it(module):
    assert "postprocessing" not in imports_of(module)[0]


def test_crown_device_is_the_lowest_layer():
    assert imports_of("crown_device")[0] <= {"_lib"}
    assert imports_of("box_pairs")[0] <= {"_lib", "crown_device"}
    assert imports_of("crown_rasters")[0] <= {"_lib", "crown_device"}


@pytest.mark.parametrize("module", ["crown_device", "box_pairs"])
def test_torch_is_imported_only_inside_functions(module):
    assert "torch" not in imports_of(module, module_level_only=True)[1]
    assert "torch" in imports_of(module)[1]
