"""CPU tier of the indexed mesh.
1. the NumPy model (tests/mesh_index_model.py) on the analytic sphere: a closed, oriented surface of genus 0 THROUGH `indices`,
   smooth normals that point outwards — the yardstick is validated before it judges anything;
2. the DEVICE CODE on the host functional model (tools/emu) against the model, byte for byte: one child process per case
   (tests/mesh_index_case.py), started side by side like those of tests/test_emu_parity.py;
3. the indexed PLY round trip."""
import json
import os
import sys

import numpy as np
import pytest

from kimera_semantics_amd.mesh import IndexedMesh, Mesh, read_ply, write_ply
from tests import mesh_case, mesh_index_case, mesh_index_model, mesh_model
from tests import test_emu_parity as EP


@pytest.fixture(scope="module")
def sphere():
    idx, t, s = mesh_case.make_field("sphere", 8)
    m = mesh_model.mesh_from_blocks(idx, t, 8, mesh_case.VOXEL, labels=s["label"])
    return m, mesh_index_model.index_of(m)


def test_model_on_an_analytic_sphere_is_closed_oriented_and_genus_0_through_indices(sphere):
    m, im = sphere
    assert m["degenerate"] == 0 and im["agree"]
    assert im["stats"] == dict(corners=16272, vertices=2714, max_corners_per_vertex=9)
    tri = im["indices"].astype(np.int64).reshape(-1, 3)
    assert im["indices"][0] == 0 and int(tri.max()) + 1 == len(im["xyz"]) == 2714
    assert im["xyz"][im["indices"]].tobytes() == m["xyz"].tobytes()
    directed = {}
    for a, b in np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).tolist():
        assert a != b
        directed[(a, b)] = directed.get((a, b), 0) + 1
    assert all(n == 1 for n in directed.values())              # every directed edge once ...
    assert all((b, a) in directed for (a, b) in directed)       # ... and its reverse once
    n_v, n_e, n_f = len(im["xyz"]), len(directed) // 2, len(tri)
    assert n_v - n_e + n_f == 2, (n_v, n_e, n_f)
    # vertices ascend by their first corner
    first = np.full(n_v, len(im["indices"]), np.int64)
    np.minimum.at(first, im["indices"].astype(np.int64), np.arange(len(im["indices"])))
    assert (np.diff(first) > 0).all()


def test_model_normals_on_the_sphere_point_outwards(sphere):
    _, im = sphere
    radial = im["xyz"].astype(np.float64) - np.array(mesh_case.SPHERE_CENTRE)
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    n = im["normals"].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-6
    assert (np.einsum("ij,ij->i", n, radial) > np.cos(np.radians(5.0))).all()


# ---- 2. the device code on the functional model: one child per case, started together by test_emu_parity's fixture ----
for _name, _spec in mesh_index_case.SPECS.items():
    EP.JOBS["test_mesh_index_device_code_on_the_host_equals_model[%s]" % _name] = (
        [sys.executable, "-m", "tests.mesh_index_case", json.dumps(_spec)], {}, 900, 30 if _spec["case"] in ("lifetime", "errors", "read_only") else 10)

emu_jobs = EP.emu_jobs


@pytest.mark.parametrize("name", sorted(mesh_index_case.SPECS))
def test_mesh_index_device_code_on_the_host_equals_model(emu_jobs, request, name):
    rc, out, err = emu_jobs.result(request.node.name)
    assert rc == 0 and "MESH_INDEX_CASE_OK" in out, out[-3000:] + err[-3000:]


def test_indexed_ply_round_trip(tmp_path, sphere):
    idx, t, s = mesh_case.make_field("two_label", 8)
    im = mesh_index_model.index_of(mesh_model.mesh_from_blocks(idx, t, 8, mesh_case.VOXEL, labels=s["label"]))
    ids = (np.arange(len(im["xyz"]), dtype=np.uint32) % 3)
    ids[::7] = 0xffffffff
    mesh = IndexedMesh(np.zeros(0, mesh_model.BLOCK_DTYPE), im["xyz"], im["normals"], im["rgba"], im["labels"], ids, im["indices"])
    path = os.path.join(tmp_path, "indexed.ply")
    write_ply(path, mesh)
    back = read_ply(path)
    assert isinstance(back, IndexedMesh)
    for name in ("xyz", "normals", "rgba", "labels", "object_ids", "indices"):
        a, b = getattr(mesh, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), name
    assert back.n_triangles == mesh.n_triangles > 0 and back.n_vertices == mesh.n_vertices < 3 * mesh.n_triangles
    with open(path, "rb") as f:
        head = f.read(600).decode("ascii", "replace")
    assert "property uchar label" in head and "property uint object_id" in head and "element vertex %d\n" % mesh.n_vertices in head
    assert "element face %d\n" % mesh.n_triangles in head and "format binary_little_endian 1.0" in head
    write_ply(path, IndexedMesh(mesh.blocks, im["xyz"][:0], im["normals"][:0], im["rgba"][:0], im["labels"][:0], ids[:0], im["indices"][:0]))
    empty = read_ply(path)
    assert isinstance(empty, IndexedMesh) and empty.n_triangles == 0 and empty.n_vertices == 0
    # the unshared form still round-trips as a Mesh
    m = sphere[0]
    write_ply(path, Mesh(m["blocks"], m["xyz"], m["normals"], m["rgba"], m["labels"]))
    assert isinstance(read_ply(path), Mesh)
