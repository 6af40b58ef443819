"""CPU tier of the semantic mesh (DESIGN.md, section "Semantic mesh").
1. the triangle table (the library's one data file) on its own: neither the kernels nor the model are involved;
2. the NumPy model (tests/mesh_model.py) on an analytic sphere: closed, oriented, genus 0 — the yardstick is validated
   before it judges anything;
3. the DEVICE CODE on the host functional model (tools/emu) against the model, bit for bit: one child process per case
   (tests/mesh_case.py), started side by side like those of tests/test_emu_parity.py;
4. the PLY round trip."""
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import pytest

from kimera_semantics_amd.mesh import EDGE_CORNERS, Mesh, load_tri_table, read_ply, write_ply
from tests import mesh_case, mesh_model
from tests import test_emu_parity as EP

CORNER = np.array([[i & 1, (i >> 1) & 1, (i >> 2) & 1] for i in range(8)])
MID2 = np.array([CORNER[a] + CORNER[b] for a, b in EDGE_CORNERS])   # edge midpoints, doubled (integers)


def triangles(table, case):
    row = [int(e) for e in table[case] if e >= 0]
    assert len(row) % 3 == 0 and all(e < 0 for e in table[case][len(row):])
    return [row[k:k + 3] for k in range(0, len(row), 3)]


def face_segments(table, case, axis, side):
    """Directed segments the case's triangles leave on the face `axis` = side, in the face's own 2-D (doubled) coordinates."""
    segs = []
    others = [a for a in range(3) if a != axis]
    for tri in triangles(table, case):
        for k in range(3):
            p, q = MID2[tri[k]], MID2[tri[(k + 1) % 3]]
            if p[axis] == 2 * side and q[axis] == 2 * side:
                segs.append((tuple(p[others]), tuple(q[others])))
    return sorted(segs)


def test_numbering_gives_shared_edges_one_direction():
    # corner number monotone in x, y, z: every edge runs from its lower corner towards +x, +y or +z
    for a, b in EDGE_CORNERS:
        d = CORNER[b] - CORNER[a]
        assert a < b and d.min() == 0 and d.sum() == 1
    assert len({(a, b) for a, b in EDGE_CORNERS}) == 12


def test_triangle_table_cases():
    table = load_tri_table()
    assert table.shape == (256, 16) and table.dtype == np.int8
    for case in range(256):
        inside = [(case >> i) & 1 for i in range(8)]
        tris = triangles(table, case)
        assert len(tris) <= 5
        crossing = {e for e, (a, b) in enumerate(EDGE_CORNERS) if inside[a] != inside[b]}
        assert {e for t in tris for e in t} == crossing, case       # (also: every vertex lies on a sign-change edge)
        assert all(len(set(t)) == 3 for t in tris), case
    assert triangles(table, 0) == [] and triangles(table, 255) == []


def test_triangle_table_adjacent_cubes_agree_on_their_shared_face():
    """On each of the six faces the segments a case leaves are those the neighbouring cube's case leaves there (in the
    opposite direction: the surface is oriented), whatever the neighbour's other four corners are."""
    table = load_tri_table()
    for axis in range(3):
        on_hi = [i for i in range(8) if CORNER[i][axis] == 1]
        for case in range(256):
            mine = face_segments(table, case, axis, 1)
            shared = [(case >> i) & 1 for i in on_hi]
            for rest in itertools.product((0, 1), repeat=4):
                other = 0
                for i, bit in zip(on_hi, shared):        # my corner i (face side 1) is the neighbour's corner i - (1 << axis)
                    other |= bit << (i - (1 << axis))
                for i, bit in zip(on_hi, rest):
                    other |= bit << i
                theirs = face_segments(table, other, axis, 0)
                assert mine == sorted((q, p) for p, q in theirs), (axis, case, other)


def _connected(corners):
    corners = set(corners)
    if not corners:
        return False
    seen, todo = set(), [next(iter(corners))]
    while todo:
        c = todo.pop()
        if c in seen:
            continue
        seen.add(c)
        todo += [c ^ (1 << k) for k in range(3) if (c ^ (1 << k)) in corners]
    return seen == corners


def test_triangle_table_orientation():
    """Normals point from the inside corners (distance < 0) to the outside ones (free space)."""
    table = load_tri_table()
    checked = 0
    for case in range(1, 255):
        ins = [i for i in range(8) if (case >> i) & 1]
        outs = [i for i in range(8) if not (case >> i) & 1]
        if not (_connected(ins) and _connected(outs)):
            continue
        towards = CORNER[outs].mean(axis=0) - CORNER[ins].mean(axis=0)
        for tri in triangles(table, case):
            p = MID2[tri] / 2.0
            n = np.cross(p[1] - p[0], p[2] - p[0])
            assert n @ towards > 0, (case, tri)
        checked += 1
    assert checked >= 100


def test_triangle_table_equals_skimage_classic_up_to_renumbering():
    luts = pytest.importorskip("skimage.measure._marching_cubes_lewiner_luts")
    import base64
    shape, text = luts.CASESCLASSIC
    ref = np.frombuffer(base64.decodebytes(text.encode()), dtype=np.int8).reshape(shape)
    # the data file's header: Bourke's corners 0..7 are corners 0,1,3,2,4,5,7,6 here, his edges 0..11 are edges
    # 0,5,1,4,2,7,3,6,8,9,11,10 here, second and third vertex of every triangle swapped
    cmap, emap = [0, 1, 3, 2, 4, 5, 7, 6], [0, 5, 1, 4, 2, 7, 3, 6, 8, 9, 11, 10]
    table = load_tri_table()
    for case in range(256):
        mine = sum(((case >> i) & 1) << cmap[i] for i in range(8))
        row = [emap[e] for e in ref[case] if e >= 0]
        want = [[row[k], row[k + 2], row[k + 1]] for k in range(0, len(row), 3)]
        assert triangles(table, mine) == want, case


def test_model_on_an_analytic_sphere_is_closed_oriented_and_genus_0():
    idx, t, s = mesh_case.make_field("sphere", 8)
    m = mesh_model.mesh_from_blocks(idx, t, 8, mesh_case.VOXEL, labels=s["label"])
    assert m["degenerate"] == 0
    xyz = m["xyz"]
    assert len(xyz) % 3 == 0 and len(xyz) // 3 > 4000
    keys = np.ascontiguousarray(xyz).view(np.uint32).reshape(-1, 3)
    _, vid = np.unique(keys, axis=0, return_inverse=True)
    tri = vid.reshape(-1, 3)
    directed = {}
    for a, b in np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).tolist():
        assert a != b
        directed[(a, b)] = directed.get((a, b), 0) + 1
    # every undirected edge is used by exactly two triangles, in opposite directions
    assert all(n == 1 for n in directed.values())
    assert all((b, a) in directed for (a, b) in directed)
    n_v, n_e, n_f = int(vid.max()) + 1, len(directed) // 2, len(tri)
    assert n_v - n_e + n_f == 2, (n_v, n_e, n_f)
    assert (np.einsum("ij,ij->i", m["normals"].astype(np.float64), xyz.astype(np.float64) - np.array(mesh_case.SPHERE_CENTRE)) > 0).all()
    # vertices lie on the sphere to within the interpolation error of a 5 cm grid
    r = np.linalg.norm(xyz.astype(np.float64) - np.array(mesh_case.SPHERE_CENTRE), axis=1)
    assert np.abs(r - mesh_case.SPHERE_RADIUS).max() < 0.2 * mesh_case.VOXEL
    assert (m["labels"] == 5).all()


def test_model_two_label_field_carries_both_labels_and_their_colours():
    from kimera_semantics_amd import synth
    idx, t, s = mesh_case.make_field("two_label", 8)
    m = mesh_model.mesh_from_blocks(idx, t, 8, mesh_case.VOXEL, labels=s["label"])
    lut = synth.default_label_colors()
    assert set(np.unique(m["labels"])) == {3, 7}
    assert (m["rgba"] == lut[m["labels"]]).all()
    left = m["xyz"][:, 0] < -mesh_case.VOXEL
    assert (m["labels"][left] == 3).all() and (m["labels"][m["xyz"][:, 0] > mesh_case.VOXEL] == 7).all()


# sha256 over indices, tsdf and sem of make_field(kind, vps), recorded before the block range was derived from a voxel extent
FIELD_HASHES = {
    ("sphere", 8): "088be9c594e903ad36df42ce937f42a9634855ea3b8dec1e874482147a1b7d7f",
    ("sphere", 16): "6316d5cc1630fe5b98102d3a1be7ef4c28994013eab022e7a7250df3af1bd932",
    ("plane", 8): "9af4fe57504fb09949a847da241cd887b4815291ed55364d6240c96e29340c54",
    ("plane", 16): "a434d11f466736490d558ce6f1f3e77c53e71db8d0ad963d1749a49210e61fc7",
    ("two_label", 8): "1965ef22f02628f8e231dcb2fd851e2b1b6154adaa935f85895b106bed7139d2",
    ("two_label", 16): "20fb8790fc3d1e3d48f9f1a43d79150709de3a24b52e2a0616cd5e9293130664",
    ("holes", 8): "7776be22da8ec57204b5ea7829e9d69b2ec073c5d8d6f30d22b6418b10ec7dd8",
    ("holes", 16): "19ac8415fca43d4aac0b1261a7c4b3d0c5783e01a2624dd338074b9c0bb71c60",
}


def test_fields_at_8_and_16_voxels_per_side_are_the_bytes_they_always_were():
    for (kind, vps), want in FIELD_HASHES.items():
        idx, t, s = mesh_case.make_field(kind, vps)
        assert hashlib.sha256(idx.tobytes() + t.tobytes() + s.tobytes()).hexdigest() == want, (kind, vps)


def test_fields_at_32_and_64_voxels_per_side_cover_whole_blocks_across_a_seam():
    for vps, blocks in ((32, 8), (64, 2)):
        for kind in ("sphere", "plane", "two_label"):
            idx, t, s = mesh_case.make_field(kind, vps)
            assert len(idx) == blocks and t.shape == s.shape == (blocks, vps ** 3), (kind, vps)
            inside = (t["distance"] < 0).any(axis=1)
            assert inside[(idx[:, 0] == -1)].any() and inside[(idx[:, 0] == 0)].any(), (kind, vps)   # the surface on both sides of x = 0
    idx, t, _ = mesh_case.make_field("holes", 32)
    assert len(idx) == 7 and 0.08 < (t["weight"] == 0).mean() < 0.12      # one block absent, a tenth of the voxels unobserved


def test_conditions_that_keep_the_upload_cases_from_being_empty_hold_for_the_model_alone():
    """The triangle floor of every upload case, with the model on the field (no library involved)."""
    for name, spec in mesh_case.SPECS.items():
        if spec["case"] != "upload" or spec["vps"] < 32:
            continue
        idx, t, s = mesh_case.make_field(spec["field"], spec["vps"])
        m = mesh_model.mesh_from_blocks(idx, t, spec["vps"], mesh_case.VOXEL, labels=s["label"])
        assert len(m["xyz"]) // 3 >= spec.get("triangles_at_least", 500), (name, len(m["xyz"]) // 3)
        if spec["field"] == "two_label":
            assert set(np.unique(m["labels"])) == {3, 7}
        if spec["field"] == "sphere":   # the same sphere at every block size: the same number of triangles
            assert len(m["xyz"]) // 3 == 5424, (name, len(m["xyz"]) // 3)


# ---- 3. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
for _name, _spec in mesh_case.SPECS.items():
    EP.JOBS["test_mesh_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.mesh_case", json.dumps(_spec)], {}, 900, 60 if _spec["case"] in ("incremental", "errors") else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(mesh_case.SPECS))
def test_mesh_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "MESH_CASE_OK" in out, out[-3000:] + err[-3000:]


def test_ply_round_trip(tmp_path):
    idx, t, s = mesh_case.make_field("two_label", 8)
    m = mesh_model.mesh_from_blocks(idx, t, 8, mesh_case.VOXEL, labels=s["label"])
    mesh = Mesh(m["blocks"], m["xyz"], m["normals"], m["rgba"], m["labels"])
    path = os.path.join(tmp_path, "mesh.ply")
    write_ply(path, mesh)
    back = read_ply(path)
    for name in ("xyz", "normals", "rgba", "labels"):
        a, b = getattr(mesh, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).tobytes(), name
    assert back.n_triangles == mesh.n_triangles > 0
    with open(path, "rb") as f:
        head = f.read(400).decode("ascii", "replace")
    assert "property uchar label" in head and "format binary_little_endian 1.0" in head
    write_ply(path, Mesh(m["blocks"][:0], m["xyz"][:0], m["normals"][:0], m["rgba"][:0], m["labels"][:0]))
    assert read_ply(path).n_triangles == 0
