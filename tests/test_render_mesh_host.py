"""Mesh geoms of the renderer, everything that needs no GPU: the loaders, the scene compile (placement, scale, mass), the
hierarchy's invariants, the CPU restatement tests/tools/render_ref.c with the hierarchy against the same with every
triangle tested (zero differing pixels), its float build against its double build (the rule of
render_cases.compare_builds, same cap), closed forms, and a mesh library that no primitive uses changing nothing."""

import os
from pathlib import Path

import numpy as np
import pytest

from render_cases import RenderRef, assert_same, compare_builds, look_at, random_scene
from render_mesh_cases import (add_meshes, awkward_scene, cube_soup, icosphere, library, random_mesh_scene, sheet, static_scene,
                               torus, with_degenerates, write_obj, write_stl_ascii, write_stl_binary, _empty_tables)

REFERENCE_MODELS = Path(os.environ.get("STAC_REFERENCE_MODELS", "/root/reference/models"))  # the reference checkout, where there is one


@pytest.fixture(scope="module")
def mrefs():
    return RenderRef("float"), RenderRef("double")


# ---- loaders ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["cube", "icosphere"])
def test_three_formats_load_the_same_triangles(tmp_path, shape):
    from stac_mjx_amd.mesh import load_mesh

    tri = cube_soup((0.3, 0.2, 0.1), (0.05, 0, 0)) if shape == "cube" else icosphere(2, 0.37)
    write_stl_binary(tmp_path / "a.stl", tri)
    write_stl_ascii(tmp_path / "b.STL", tri)
    write_obj(tmp_path / "c.obj", tri)
    write_obj(tmp_path / "d.obj", tri, negative=True)
    write_obj(tmp_path / "e.obj", tri, extras=False)
    for name in ("a.stl", "b.STL", "c.obj", "d.obj", "e.obj"):
        got = load_mesh(tmp_path / name)
        assert got.dtype == np.float32 and got.shape == tri.shape, name
        np.testing.assert_array_equal(got, tri, err_msg=name)


def test_obj_polygons_are_fan_triangulated(tmp_path):
    from stac_mjx_amd.mesh import load_mesh

    (tmp_path / "q.obj").write_text("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 2 0\nvn 0 0 1\nf 1//1 2//1 3//1 4//1 5//1\nl 1 2\nf -5 -4 -3 -2\n")
    got = load_mesh(tmp_path / "q.obj")
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 2, 0]], np.float32)
    want = v[[[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 1, 2], [0, 2, 3]]]
    np.testing.assert_array_equal(got, want)


def test_bad_files_are_refused(tmp_path):
    from stac_mjx_amd.mesh import MeshError, load_mesh

    tri = icosphere(1)
    write_stl_binary(tmp_path / "ok.stl", tri)
    data = (tmp_path / "ok.stl").read_bytes()
    (tmp_path / "cut.stl").write_bytes(data[:-30])  # truncated binary
    write_stl_ascii(tmp_path / "ok_ascii.stl", tri)
    text = (tmp_path / "ok_ascii.stl").read_text()
    (tmp_path / "cut_ascii.stl").write_text(text[: len(text) // 2])  # no endsolid
    (tmp_path / "idx.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    (tmp_path / "neg.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -4\n")
    (tmp_path / "zero.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n")
    (tmp_path / "empty.obj").write_text("v 0 0 0\n")
    (tmp_path / "m.msh").write_bytes(b"\0" * 64)
    for name in ("cut.stl", "cut_ascii.stl", "idx.obj", "neg.obj", "zero.obj", "empty.obj", "m.msh", "missing.stl"):
        with pytest.raises(MeshError):
            load_mesh(tmp_path / name)


def test_every_mesh_file_of_the_reference_loads():
    from stac_mjx_amd.mesh import load_mesh

    if not REFERENCE_MODELS.exists():
        pytest.skip("the reference's model directory is not on this machine")
    files = sorted(p for p in REFERENCE_MODELS.rglob("*") if p.suffix.lower() in (".stl", ".obj"))
    assert files
    total = 0
    for p in files:
        tri = load_mesh(p)
        assert np.isfinite(tri).all(), p
        if p.suffix.lower() == ".stl":
            data = p.read_bytes()
            stated = int.from_bytes(data[80:84], "little") if len(data) == 84 + 50 * int.from_bytes(data[80:84], "little") else data.count(b"endfacet")
        else:
            stated = sum(max(len(l.split()) - 3, 0) for l in p.read_text(errors="replace").splitlines() if l.startswith("f "))
        assert len(tri) == stated, (p, len(tri), stated)
        total += len(tri)
    print(f"{len(files)} mesh files, {total} triangles")


# ---- scene compile ------------------------------------------------------------------------------------------------------------
MESH_XML = """
<mujoco>
  <compiler meshdir="m"/>
  <default>
    <mesh scale="0.1 0.1 0.1"/>
    <default class="boxy"><geom type="box" size="0.01 0.01 0.01"/></default>
  </default>
  <asset>
    <mesh name="cube" file="cube.stl"/>
    <mesh file="ico.obj" scale="1 2 3" refpos="1 0 0" refquat="0.7071067811865476 0 0 0.7071067811865476"/>
    <mesh name="gone" file="gone.stl"/>
    <mesh name="other" file="thing.msh"/>
  </asset>
  <worldbody>
    <geom name="floor" type="plane" size="1 1 0.1"/>
    <body name="a" pos="0 0 1"><freejoint/>
      <geom name="g_cube" mesh="cube" pos="0.5 0 0" density="2000"/>
      <geom name="g_sized" mesh="cube" size="0.3"/>
      <geom name="g_ico" mesh="ico" group="1" mass="3"/>
      <geom name="g_box" class="boxy" mesh="cube"/>
      <geom name="g_gone" type="mesh" mesh="gone"/>
      <geom name="g_other" mesh="other"/>
      <geom name="g_undeclared" mesh="nope"/>
    </body>
  </worldbody>
</mujoco>"""


def _write_model(tmp_path):
    (tmp_path / "m").mkdir()
    cube = cube_soup((1.0, 1.0, 1.0), (3.0, 0.0, 0.0))  # side 2, off centre
    write_stl_binary(tmp_path / "m" / "cube.stl", cube)
    ico = icosphere(1)
    write_obj(tmp_path / "m" / "ico.obj", ico)
    (tmp_path / "model.xml").write_text(MESH_XML)
    return cube, ico


def test_scene_compile_places_scales_and_weighs_meshes(tmp_path):
    from stac_mjx_amd.mjcf import GEOM_BOX, GEOM_MESH, compile_render_scene

    cube, ico = _write_model(tmp_path)
    msgs = []
    s = compile_render_scene(tmp_path / "model.xml", log=msgs.append)
    assert s.geom_names == ["floor", "g_cube", "g_sized", "g_ico", "g_box"]
    assert s.n_skipped == 3 and len(msgs) == 1 and "3 mesh" in msgs[0]
    # mesh without type -> mesh geom (not a sphere of its size); a class that sets a type wins
    assert list(s.geom_type[1:]) == [GEOM_MESH, GEOM_MESH, GEOM_MESH, GEOM_BOX]
    assert list(s.geom_mesh) == [-1, 0, 0, 1, -1] and [m.name for m in s.meshes] == ["cube", "ico"]
    # default-class scale 0.1, meshdir, name = the file's stem
    got = np.sort(s.meshes[0].tris.reshape(-1, 3), axis=0)
    np.testing.assert_allclose(got, np.sort((cube * np.float32(0.1)).reshape(-1, 3), axis=0), rtol=1e-6)
    # own scale, refpos, refquat: scale * rotate(conj(q), v - refpos); q = 90 degrees about z: conj takes x -> -y, y -> x
    v = ico.reshape(-1, 3).astype(np.float64) - [1, 0, 0]
    want = np.stack([v[:, 1], -v[:, 0], v[:, 2]], 1) * [1, 2, 3]
    got = s.meshes[1].tris.reshape(-1, 3)
    np.testing.assert_allclose(got[np.lexsort(got.T)], want[np.lexsort(want.astype(np.float32).T)], atol=1e-6)
    # mass = density x volume at the volume centroid; `mass` wins.  Cube of side 0.2 centred at x = 0.3 in the geom frame.
    np.testing.assert_allclose(s.geom_mass[1], 2000 * 0.2**3, rtol=1e-6)
    np.testing.assert_allclose(s.geom_mass[2], 1000 * 0.2**3, rtol=1e-6)
    assert s.geom_mass[3] == 3.0
    np.testing.assert_allclose(s.meshes[0].centroid, [0.3, 0, 0], atol=1e-7)
    m = s.geom_mass[1:5]
    c = np.array([[0.8, 0, 0], [0.3, 0, 0], s.meshes[1].centroid, [0, 0, 0]])
    np.testing.assert_allclose(s.body_mass[1], m.sum(), rtol=1e-12)
    np.testing.assert_allclose(s.body_ipos[1], (m[:, None] * c).sum(0) / m.sum(), atol=1e-9)


def test_scale_factor_scales_every_mesh_and_from_string_needs_asset_dir(tmp_path):
    from stac_mjx_amd.mjcf import compile_render_scene

    cube, _ = _write_model(tmp_path)
    s1 = compile_render_scene(tmp_path / "model.xml", log=lambda *a: None)
    s2 = compile_render_scene(tmp_path / "model.xml", scale=0.5, log=lambda *a: None)
    np.testing.assert_allclose(s2.meshes[0].tris, s1.meshes[0].tris * np.float32(0.5), rtol=1e-6)
    np.testing.assert_allclose(s2.meshes[0].volume, s1.meshes[0].volume / 8, rtol=1e-6)
    msgs = []
    s3 = compile_render_scene(MESH_XML, from_string=True, log=msgs.append)
    assert s3.n_skipped == 6 and len(s3.meshes) == 0 and len(msgs) == 1
    s4 = compile_render_scene(MESH_XML, from_string=True, asset_dir=tmp_path, log=lambda *a: None)
    assert s4.n_skipped == 3 and len(s4.meshes) == 2


def test_render_tables_emit_mesh_geoms_in_document_order(tmp_path):
    from stac_mjx_amd.mjcf import compile_render_scene
    from stac_mjx_amd.render import FLAG_TRANSPARENT, render_tables

    _write_model(tmp_path)
    s = compile_render_scene(tmp_path / "model.xml", log=lambda *a: None)
    t = render_tables(s, np.ones((2, 4)), 0.005)
    assert t["names"] == ["floor", "g_cube", "g_sized", "g_box"]  # group 1 is off by default
    assert list(t["prim_type"]) == [0, 7, 7, 6] and list(t["meshes"]["prim_mesh"]) == [-1, 0, 0, -1]
    assert list(t["prim_flags"] & FLAG_TRANSPARENT) == [0, 1, 1, 1]
    assert len(t["meshes"]["node_offset"]) == 2  # only the mesh that is drawn is uploaded
    t = render_tables(s, np.ones((2, 4)), 0.005, geom_groups=(0, 1, 2))
    assert t["names"] == ["floor", "g_cube", "g_sized", "g_ico", "g_box"] and list(t["meshes"]["prim_mesh"]) == [-1, 0, 0, 1, -1]


# ---- hierarchy ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tri", [icosphere(0), icosphere(3), torus(), sheet(), with_degenerates(cube_soup()), icosphere(0)[:1], icosphere(0)[:5]],
                         ids=["ico0", "ico3", "torus", "sheet", "cube+degenerate", "one", "five"])
def test_hierarchy_invariants(tri):
    from stac_mjx_amd.mesh import LEAF_TRIS, build_bvh

    ts, box, link = build_bvh(tri)
    ts2, box2, link2 = build_bvh(tri.copy())
    for a, b in ((ts, ts2), (box, box2), (link, link2)):
        np.testing.assert_array_equal(a, b)  # deterministic
    assert sorted(map(bytes, ts)) == sorted(map(bytes, tri))  # a permutation of the input
    NN = len(box)
    leaf = link[:, 2] > 0
    cover = np.zeros(len(ts), int)
    for first, count in link[leaf, 1:]:
        assert 1 <= count <= LEAF_TRIS
        cover[first:first + count] += 1
    assert (cover == 1).all()  # every triangle in exactly one leaf
    n = np.arange(NN)
    assert (link[:, 0] > n).all() and (link[:, 0] <= NN).all() and link[0, 0] == NN  # strictly forward
    assert (link[leaf, 0] == n[leaf] + 1).all()
    for k in range(NN):  # every box contains its subtree's triangles and boxes
        sub = np.arange(k, link[k, 0])
        assert (box[sub, :3] >= box[k, :3]).all() and (box[sub, 3:] <= box[k, 3:]).all()
        for first, count in link[sub][link[sub, 2] > 0][:, 1:]:
            v = ts[first:first + count].reshape(-1, 3)
            assert (v >= box[k, :3]).all() and (v <= box[k, 3:]).all()
        if not leaf[k]:  # an inner node's children: k + 1 and the skip of k + 1, ending where k ends
            assert link[link[k + 1, 0], 0] == link[k, 0]


# ---- the reference: hierarchy against brute force --------------------------------------------------------------------------------
def test_hierarchy_equals_brute_force_on_awkward_scene(mrefs):
    args = awkward_scene(3) + (160, 120)
    args = args[:5] + (False,) + args[5:]
    a = mrefs[0].render(*_args(args))
    b = mrefs[0].render(*_args(args), brute=True)
    assert_same(a[:3], b[:3], "awkward scene")
    seg = a[1]
    assert (seg[0] >= 0).all()  # inside the shell every ray hits something: the inside of a mesh is drawn
    assert (seg[0] == 1).any() and (seg[1] == 2).any() and (seg[2] == 2).any()  # the sheet from above and from below
    assert (seg[4] == 3).any() and not (seg[4] == 4).any()  # coincident opaque cubes: the lower id wins
    assert (seg[3] == 2).sum() < 0.02 * seg[3].size  # along its plane the flat sheet is (nearly) invisible


def _args(a):
    """(tables, xpos, xquat, kp, markers, show, cams, tanh, W, H) -> the argument list of RenderRef.render."""
    t, xpos, xquat, kp, markers, show, cams, tanh, W, H = a
    return t, xpos.shape[1], xpos, xquat, kp, markers, show, cams, tanh, W, H


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_hierarchy_equals_brute_force_on_random_scenes(mrefs, seed):
    t, xpos, xquat, kp, markers, cams, tanh = random_mesh_scene(seed, 20, 7, n_mesh=16, subdivs=(0, 2, 4, 5), n_frames=2)
    for W, H, show in ((160, 120, True), (97, 61, False)):
        a = mrefs[0].render(t, 20, xpos, xquat, kp, markers, show, cams, tanh, W, H)
        b = mrefs[0].render(t, 20, xpos, xquat, kp, markers, show, cams, tanh, W, H, brute=True)
        assert_same(a[:3], b[:3], f"seed {seed} {W}x{H}")
        assert np.isin(a[1], np.flatnonzero(t["prim_type"] == 7)).any()  # meshes are in the picture


# ---- float build against double build ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_f32_checker_matches_f64_on_coarse_mesh_scenes(mrefs, seed):
    """Coarse meshes (icosphere subdivision at most 3 at 320 x 240: the share of rays within rounding of an edge grows with
    the edge length per image area), among the spheres and boxes that ``random_scene`` adds by hand (the see-through stack,
    the primitives around the camera) and the keypoints, markers and segments.  The random primitives are left out
    (``n_static=0``): their float / double agreement is the subject of tests/test_render_host.py with its own scenes, and
    with them one cylinder pixel of seed 1 (no mesh on its ray) differs by 1.7e-5 in depth, above the 1e-5 that
    ``compare_builds`` allows, without being flagged by the cylinder's conditions."""
    t, xpos, xquat, kp, markers, cams, tanh = random_mesh_scene(seed, 20, 7, n_mesh=14, subdivs=(0, 1, 2, 3), n_static=0, n_frames=2)
    for show in (False, True):
        compare_builds(mrefs, (t, 20, xpos, xquat, kp, markers, show, cams, tanh, 320, 240))


def test_f32_checker_matches_f64_on_awkward_scene(mrefs):
    a = awkward_scene(3)
    args = _args(a[:5] + (False,) + a[5:] + (320, 240))
    # not here: the frame that looks along the flat sheet's plane (all grazing rays) and the two frames of the coincident
    # cubes (every pixel of theirs is a tie, which the double build flags, rightly): the double build alone puts them above
    # the cap.  They are checked against brute force above, and float-to-kernel on the GPU.
    keep = [0, 1, 2, 5]
    args = args[:2] + tuple(x[keep] for x in args[2:6]) + (args[6], args[7][keep]) + args[8:]
    compare_builds(mrefs, args)


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def test_cube_soup_is_the_box_primitive(mrefs):
    from stac_mjx_amd.mesh import make_mesh

    h = (0.11, 0.07, 0.05)
    rng = np.random.default_rng(3)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    pos = [0.1, -0.2, 0.4]
    cams = [look_at([0.6, 0.5, 0.9], pos), look_at([-0.4, 0.1, 0.3], pos)]
    tm = static_scene([make_mesh("cube", cube_soup(h))], [(0, pos, q, [0.5, 0.6, 0.7, 1], 0)], cams)
    tb = _empty_tables()
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    tb.update(prim_type=np.array([6], np.int32), prim_body=np.zeros(1, np.int32), prim_flags=np.zeros(1, np.int32), prim_size=f32([h]),
              prim_pos=f32([pos]), prim_quat=f32([q]), prim_rgba=f32([[0.5, 0.6, 0.7, 1]]), prim_rgb2=f32(np.zeros((1, 3))),
              prim_texrepeat=f32(np.ones((1, 2))), names=["box"])
    for ref in mrefs:
        a = ref.render(tm[0], 1, *tm[1:5], False, tm[5], tm[6], 320, 240)
        b = ref.render(tb, 1, *tm[1:5], False, tm[5], tm[6], 320, 240)
        # the silhouettes agree except where a ray grazes an edge of the cube (flagged by either picture)
        amb = (a[3] | b[3]).astype(bool)
        assert amb.mean() < 0.01
        assert ((a[1] != b[1]) & ~amb).sum() == 0 and (a[1] == 0).sum() > 2000
        hit = (a[1] == 0) & (b[1] == 0) & ~amb
        rel = np.abs(a[2][hit].astype(np.float64) - b[2][hit]) / b[2][hit]
        print("cube soup vs box: max relative depth difference", rel.max())
        assert rel.max() <= 1e-6
        assert np.abs(a[0].astype(int) - b[0].astype(int))[hit].max() <= 1  # flat shading of a box is the box's shading


def test_icosphere_silhouette_lies_between_inscribed_and_circumscribed_spheres(mrefs):
    from stac_mjx_amd.mesh import make_mesh

    R = 0.2
    tri = icosphere(2, R)
    # inscribed radius: the smallest distance of a face plane from the centre
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float64)
    r_in = float(np.min(np.abs(np.einsum("ij,ij->i", n, tri[:, 0])) / np.linalg.norm(n, axis=1)))
    assert 0.9 * R < r_in < R
    pos = [0.0, 0.0, 0.5]
    cams = [look_at([0.9, 0.3, 0.8], pos)]
    tm = static_scene([make_mesh("ico", tri)], [(0, pos, [1, 0, 0, 0], [0.5, 0.6, 0.7, 1], 0)], cams)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    pics = {}
    for name, rad in (("in", r_in * (1 - 1e-5)), ("out", R * (1 + 1e-5))):
        tb = _empty_tables()
        tb.update(prim_type=np.array([2], np.int32), prim_body=np.zeros(1, np.int32), prim_flags=np.zeros(1, np.int32),
                  prim_size=f32([[rad, 0, 0]]), prim_pos=f32([pos]), prim_quat=f32([[1, 0, 0, 0]]), prim_rgba=f32([[0.5, 0.6, 0.7, 1]]),
                  prim_rgb2=f32(np.zeros((1, 3))), prim_texrepeat=f32(np.ones((1, 2))), names=["s"])
        pics[name] = mrefs[1].render(tb, 1, *tm[1:5], False, tm[5], tm[6], 320, 240)
    a = mrefs[1].render(tm[0], 1, *tm[1:5], False, tm[5], tm[6], 320, 240)
    mesh, inner, outer = a[1] == 0, pics["in"][1] == 0, pics["out"][1] == 0
    assert inner.sum() > 3000 and (inner & ~mesh).sum() == 0 and (mesh & ~outer).sum() == 0
    both = mesh & inner
    assert (a[2][both] <= pics["in"][2][both] * (1 + 1e-6)).all() and (a[2][both] >= pics["out"][2][both] * (1 - 1e-6)).all()


# ---- mesh-free scenes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("real", ["float", "double"])
def test_an_unused_mesh_library_changes_nothing(mrefs, seed, real):
    """Mesh-free tables as they are (``nmesh = 0``, null mesh pointers) and with a ``meshes`` entry that no primitive uses
    (``nmesh > 0``, ``prim_mesh`` all -1): the same bytes in every output."""
    ref = mrefs[0] if real == "float" else mrefs[1]
    t, xpos, xquat, kp, markers, cams, tanh = random_scene(seed, 67, 23, n_frames=2)
    tm = add_meshes(t, library((0, 2)), [], [], np.zeros((0, 3)), np.zeros((0, 4)), np.zeros((0, 4)), [])
    assert "meshes" not in t and len(tm["meshes"]["node_offset"]) > 1 and (tm["meshes"]["prim_mesh"] == -1).all()
    for show in (False, True):
        a = ref.render(t, 67, xpos, xquat, kp, markers, show, cams, tanh, 160, 120)
        b = ref.render(tm, 67, xpos, xquat, kp, markers, show, cams, tanh, 160, 120)
        assert_same(a[:3], b[:3], f"seed {seed} {real} show_error={show}")
        np.testing.assert_array_equal(a[3], b[3])
