"""The semantic mesh as HipIntegrator.mesh() returns it (and its indexed view, HipIntegrator.mesh_index()), their PLY forms, and
the marching-cubes triangle table.

The table exists ONCE, as the data file csrc/ks_mc_tri_table.inc: the device code includes it as an array initialiser,
load_tri_table() parses the same file (for the tests' NumPy model)."""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
TRI_TABLE_PATH = os.path.join(_HERE, "csrc", "ks_mc_tri_table.inc")

# corner i sits at (i & 1, (i >> 1) & 1, (i >> 2) & 1); edge e joins EDGE_CORNERS[e] = (a, b), a < b (the data file's header)
EDGE_CORNERS = ((0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7))


def load_tri_table() -> np.ndarray:
    """(256, 16) int8: per case up to five triangles as edge triples, -1 terminated."""
    vals = []
    with open(TRI_TABLE_PATH) as f:
        for line in f:
            line = line.split("//")[0]
            vals += [int(t) for t in line.replace(",", " ").split()]
    t = np.array(vals, dtype=np.int8)
    assert t.size == 256 * 16, t.size
    return t.reshape(256, 16)


@dataclass
class Mesh:
    blocks: np.ndarray    # binding.MESH_BLOCK_DTYPE: block index, first_vertex, n_vertices (blocks with vertices, ascending)
    xyz: np.ndarray       # (N, 3) f32, three vertices per triangle
    normals: np.ndarray   # (N, 3) f32, the triangle's normal at each of its vertices
    rgba: np.ndarray      # (N, 4) u8
    labels: np.ndarray    # (N,) u8
    stats: dict = field(default_factory=dict)

    @property
    def n_triangles(self) -> int:
        return len(self.xyz) // 3


@dataclass
class IndexedMesh:
    """The stored mesh with shared vertices (ks_mesh_index): vertices ascend by the first corner that references them."""
    blocks: np.ndarray      # the directory of the stored mesh: first_vertex / n_vertices address `indices` (corners), not the vertices
    xyz: np.ndarray         # (V, 3) f32
    normals: np.ndarray     # (V, 3) f32, from the integer sums of the incident triangles' normals
    rgba: np.ndarray        # (V, 4) u8
    labels: np.ndarray      # (V,) u8
    object_ids: np.ndarray  # (V,) u32, binding.KS_OBJECT_NONE where no object
    indices: np.ndarray     # (C,) u32: the vertex of every corner; triangle k = indices[3k : 3k + 3]
    stats: dict = field(default_factory=dict)

    @property
    def n_triangles(self) -> int:
        return len(self.indices) // 3

    @property
    def n_vertices(self) -> int:
        return len(self.xyz)


_PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                        ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1"), ("label", "u1")])
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
_PLY_NAMES = {"<f4": "float", "u1": "uchar", "|u1": "uchar"}


_PLY_VERTEX_INDEXED = np.dtype(_PLY_VERTEX.descr + [("object_id", "<u4")])
_PLY_NAMES_INDEXED = dict(_PLY_NAMES, **{"<u4": "uint"})


def _write_ply_indexed(path, mesh: IndexedMesh) -> None:
    v = np.zeros(len(mesh.xyz), dtype=_PLY_VERTEX_INDEXED)
    for k, name in enumerate(("x", "y", "z")):
        v[name] = mesh.xyz[:, k]
        v["n" + name] = mesh.normals[:, k]
    for k, name in enumerate(("red", "green", "blue", "alpha")):
        v[name] = mesh.rgba[:, k]
    v["label"] = mesh.labels
    v["object_id"] = mesh.object_ids
    f = np.zeros(len(mesh.indices) // 3, dtype=_PLY_FACE)
    f["n"] = 3
    f["v"] = np.asarray(mesh.indices).astype(np.int32).reshape(-1, 3)
    head = ["ply", "format binary_little_endian 1.0",
            "comment indexed semantic mesh: shared vertices, label = arg-max class of the voxel containing the vertex, object_id 4294967295 = none",
            "element vertex %d" % len(v)]
    head += ["property %s %s" % (_PLY_NAMES_INDEXED[_PLY_VERTEX_INDEXED[name].str], name) for name in _PLY_VERTEX_INDEXED.names]
    head += ["element face %d" % len(f), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())


def write_ply(path, mesh) -> None:
    """Binary little-endian PLY.  A Mesh: vertex x y z nx ny nz red green blue alpha label, face = three sequential indices.
    An IndexedMesh: the shared vertices with an object_id property after the label, faces referencing them."""
    if isinstance(mesh, IndexedMesh):
        return _write_ply_indexed(path, mesh)
    n = len(mesh.xyz)
    v = np.zeros(n, dtype=_PLY_VERTEX)
    for k, name in enumerate(("x", "y", "z")):
        v[name] = mesh.xyz[:, k]
        v["n" + name] = mesh.normals[:, k]
    for k, name in enumerate(("red", "green", "blue", "alpha")):
        v[name] = mesh.rgba[:, k]
    v["label"] = mesh.labels
    f = np.zeros(n // 3, dtype=_PLY_FACE)
    f["n"] = 3
    f["v"] = np.arange(n, dtype=np.int32).reshape(-1, 3)
    head = ["ply", "format binary_little_endian 1.0", "comment semantic mesh: label = arg-max class of the voxel containing the vertex",
            "element vertex %d" % n]
    head += ["property %s %s" % (_PLY_NAMES[_PLY_VERTEX[name].str], name) for name in _PLY_VERTEX.names]
    head += ["element face %d" % len(f), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())


def read_ply(path):
    """Reads what write_ply wrote (those two layouts only): a Mesh, or an IndexedMesh when the vertices carry an object_id."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0", head[:2]
    nv = nf = None
    props = []
    for line in head:
        w = line.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        elif w[:2] == ["element", "face"]:
            nf = int(w[2])
        elif w[:1] == ["property"] and w[1] != "list":
            props.append(w[2])
    no_blocks = np.zeros(0, dtype=[("block", "<i4", (3,)), ("first_vertex", "<u4"), ("n_vertices", "<u4")])
    if tuple(props) == _PLY_VERTEX_INDEXED.names:
        v = np.frombuffer(data, dtype=_PLY_VERTEX_INDEXED, count=nv, offset=end)
        f = np.frombuffer(data, dtype=_PLY_FACE, count=nf, offset=end + nv * _PLY_VERTEX_INDEXED.itemsize)
        assert (f["n"] == 3).all()
        return IndexedMesh(no_blocks, np.stack([v["x"], v["y"], v["z"]], axis=1), np.stack([v["nx"], v["ny"], v["nz"]], axis=1),
                           np.stack([v["red"], v["green"], v["blue"], v["alpha"]], axis=1), v["label"].copy(), v["object_id"].copy(),
                           f["v"].reshape(-1).astype(np.uint32))
    assert tuple(props) == _PLY_VERTEX.names, props
    v = np.frombuffer(data, dtype=_PLY_VERTEX, count=nv, offset=end)
    f = np.frombuffer(data, dtype=_PLY_FACE, count=nf, offset=end + nv * _PLY_VERTEX.itemsize)
    assert (f["n"] == 3).all() and (f["v"].reshape(-1) == np.arange(nv)).all()
    xyz = np.stack([v["x"], v["y"], v["z"]], axis=1)
    nrm = np.stack([v["nx"], v["ny"], v["nz"]], axis=1)
    rgba = np.stack([v["red"], v["green"], v["blue"], v["alpha"]], axis=1)
    return Mesh(np.zeros(0, dtype=[("block", "<i4", (3,)), ("first_vertex", "<u4"), ("n_vertices", "<u4")]), xyz, nrm, rgba,
                v["label"].copy())
