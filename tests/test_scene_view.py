"""The one scene view and the one quantized-node buffer on the CPU (tests/native/path_harness.cpp): pack_qnodes
against a restatement of the buffer's layout, and the view that view_set_scene / view_set_accel (pt_accel.hpp) fill
from a realized scene: its pointers, counts and bounds, and the kernel builds scene_builds() asks for."""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import pytest

from conftest import native_lib, scene_text

ROOT = Path(__file__).resolve().parent.parent
NATIVE = ROOT / "tests" / "native"
sys.path.insert(0, str(ROOT / "scenes"))
import make_scenes  # noqa: E402

BIG = 1 << 15  # BIG_BVH_NODES (pt_dims.hpp): nodes per layout from which build_accel makes the quantized nodes


@pytest.fixture(scope="module")
def H():
    subprocess.run(["make", "-s", "-C", str(NATIVE)], check=True)
    L = C.CDLL(native_lib("libpath.so"))
    L.h_scene_new.restype = C.c_void_p
    L.h_scene_new.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_uint64]
    L.h_scene_free.argtypes = [C.c_void_p]
    L.h_pack_check.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.h_pack_empty_without_qnodes.argtypes = [C.c_void_p]
    L.h_view_check.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    return L


class Host:
    def __init__(self, H, text, random_spheres=True):
        raw = text.encode()
        self.H, self.h = H, H.h_scene_new(raw, len(raw), 1 if random_spheres else 0, 1)
        assert self.h

    def __del__(self):
        self.H.h_scene_free(self.h)

    def pack(self):
        out = (C.c_uint64 * 4)()
        return self.H.h_pack_check(self.h, out), list(out)

    def view(self):
        ints, bounds = (C.c_int * 11)(), (C.c_float * 2)()
        return self.H.h_view_check(self.h, ints, bounds), list(ints), list(bounds)


def qleaf_offset(n):
    """pt_types.hpp: the grid's line, then the eight layouts and one node of padding, rounded up to a line."""
    return 64 + ((8 * n + 1) * 16 + 63) // 64 * 64


def one_node_scene():
    """More JSON shapes than the uniform list takes (LIN_MAX = 32), all but one of them Toruses (which never enter
    the BVH): the tree is the one sphere's leaf."""
    tr = lambda x: {"translate": [x, 0, 0], "rotate": [0, 0, 0], "scale": [1, 1, 1]}  # noqa: E731
    shapes = [{"type": "Torus", "name": "T%d" % i, "radius": 0.5, "tube_radius": 0.1, "transform": tr(2.0 * i),
               "material": "M"} for i in range(32)]
    shapes.append({"type": "Sphere", "name": "S", "transform": tr(-3.0), "material": "M"})
    return json.dumps({
        "camera": {"position": [0, 0, -5], "direction": [0, 0, 1], "up": [0, 1, 0], "fov": 40, "focal_length": 1},
        "shapes": shapes, "materials": {"M": {"type": "EmptyMaterial"}}, "background": [0, 0, 0]})


BIG_SPHERES = BIG // 2 + 1  # one leaf per sphere: 2 n - 1 nodes per layout


@pytest.fixture(scope="module")
def big_tree(H):
    """The random-sphere field (C5's recipe) with BIG_SPHERES small spheres: its full 128 x 128 grid and one more."""
    js = make_scenes.synthetic(BIG_SPHERES - 1)
    extra = json.loads(json.dumps(js["shapes"][-1]))
    extra["name"] = "Extra"
    extra["transform"]["translate"][1] += 0.5
    js["shapes"].append(extra)
    assert len(js["shapes"]) == 1 + BIG_SPHERES  # (the ground sphere joins the uniform list)
    return Host(H, json.dumps(js), random_spheres=False)


def check_pack(host, nodes=None):
    rc, (nbytes, per_octant, qnodes, records) = host.pack()
    assert rc == 0
    assert qnodes == 8 * per_octant and qnodes > 0
    assert nbytes == qleaf_offset(per_octant) + records * 64
    if nodes is not None:
        assert per_octant == nodes
    assert host.H.h_pack_empty_without_qnodes(host.h) == 1
    return per_octant, records


def test_pack_qnodes_small_tree_forced(H, cornell_text):
    """A tree below BIG_BVH_NODES (the Cornell box's random spheres), its quantized nodes made by build_qnodes."""
    per_octant, records = check_pack(Host(H, cornell_text))
    assert 1 < per_octant < BIG and records > 0


def test_pack_qnodes_smallest_large_tree(big_tree):
    """The smallest tree of the random-sphere field that build_accel itself quantizes: one sphere fewer stays below
    BIG_BVH_NODES nodes per layout."""
    per_octant, records = check_pack(big_tree, 2 * BIG_SPHERES - 1)
    assert per_octant >= BIG > 2 * (BIG_SPHERES - 1) - 1
    assert records == BIG_SPHERES  # every leaf holds one sphere


def test_pack_qnodes_one_node_tree(H):
    """The single-leaf tree: the padding node directly follows eight one-node layouts, and the records start on the
    next line boundary."""
    host = Host(H, one_node_scene(), random_spheres=False)
    per_octant, records = check_pack(host, 1)
    assert records == 1 and qleaf_offset(1) == 64 + 192
    assert host.pack()[1][0] == 64 + 192 + 64


def test_pack_qnodes_empty_without_a_tree(H, cornell_text):
    """No BVH at all (every shape in the uniform or the marched list): nothing to pack, and a null qnodes."""
    host = Host(H, cornell_text, random_spheres=False)
    assert host.pack() == (0, [0, 0, 0, 0])
    assert host.view()[0] == 0


@pytest.mark.parametrize("which", ["textured", "big_tree"])
def test_view_pointers_counts_and_bounds(H, big_tree, which):
    host = Host(H, scene_text("textured.json")) if which == "textured" else big_tree
    bad, ints, bounds = host.view()
    assert bad == 0  # every pointer non-null exactly when its vector is non-empty
    nnodes, a_nnodes, nlin, a_nlin, nmarch, a_nmarch, nmats, s_nmats, ext, fkind, v_ext = ints
    assert (nnodes, nlin, nmarch, nmats) == (a_nnodes, a_nlin, a_nmarch, s_nmats)
    assert nnodes > 0 and nmats > 0 and v_ext == ext
    assert bounds[0] == bounds[1] > 0.0
    if which == "textured":
        assert (ext, fkind) == (1, -1) and nmarch == 1  # textures; its marched shape is a Cushion
    else:
        assert (ext, fkind) == (0, 0) and nnodes >= BIG and nlin == 1  # the ground sphere is the uniform list


@pytest.mark.parametrize("name,ext,fkind", [
    ("torus.json", 1, 0),        # a Torus: the extended builds; nothing marched
    ("noise.json", 1, 0),        # a noise texture
    ("cornell_box.json", 0, 0),  # solid colours, a Heart: the Heart-only builds
    ("spheres.json", 0, 0),      # two Hearts
    ("marched.json", 0, -1),     # Sine, Star, ... : any function
])
def test_scene_builds(H, name, ext, fkind):
    bad, ints, _ = Host(H, scene_text(name), random_spheres=False).view()
    assert bad == 0
    assert (ints[8], ints[9], ints[10]) == (ext, fkind, ext)
