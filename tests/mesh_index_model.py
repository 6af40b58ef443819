"""The yardstick of the indexed-mesh tests: a NumPy restatement of DESIGN.md §18, written from the contract and not from the
kernels.  index_of(mesh) takes an UNSHARED mesh (a kimera_semantics_amd.mesh.Mesh, or the dict of tests/mesh_model.py) and
returns every output array of ks_mesh_index except the object ids (they come from ks_objects_query; tests compare them there)."""
import numpy as np

F = np.float32


def _get(mesh, name):
    return mesh[name] if isinstance(mesh, dict) else getattr(mesh, name)


def index_of(mesh):
    xyz = np.ascontiguousarray(_get(mesh, "xyz"), dtype=F).reshape(-1, 3)
    nrm = np.ascontiguousarray(_get(mesh, "normals"), dtype=F).reshape(-1, 3)
    rgba = np.ascontiguousarray(_get(mesh, "rgba"), dtype=np.uint8).reshape(-1, 4)
    labels = np.ascontiguousarray(_get(mesh, "labels"), dtype=np.uint8).reshape(-1)
    n_corners = len(xyz)
    if n_corners == 0:
        return dict(xyz=np.zeros((0, 3), F), normals=np.zeros((0, 3), F), rgba=np.zeros((0, 4), np.uint8), labels=np.zeros(0, np.uint8),
                    indices=np.zeros(0, np.uint32), stats=dict(corners=0, vertices=0, max_corners_per_vertex=0), agree=True)
    # 1 + 2: identity by bits; vertices ascend by the smallest corner that references them
    keys = xyz.view(np.uint32).reshape(-1, 3)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    indices = rank[inverse]
    first_corner = np.sort(first)
    n_vertices = len(first_corner)
    # 3: attributes of the first corner (and whether every corner of a group agrees: the tests assert it)
    agree = bool((rgba == rgba[first_corner][indices]).all() and (labels == labels[first_corner][indices]).all())
    # 4: integer sums of the face normals, half to even; exact in f32 below 256 corners per vertex
    q = np.rint(nrm * F(65536.0)).astype(np.int32)
    sums = np.zeros((n_vertices, 3), np.int32)
    np.add.at(sums, indices, q)
    s = sums.astype(F)
    ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    assert s.dtype == F and ln.dtype == F
    with np.errstate(invalid="ignore", divide="ignore"):
        normals = np.where((ln > F(0))[:, None], s / ln[:, None], F(0)).astype(F)
    valence = np.bincount(indices, minlength=n_vertices)
    return dict(xyz=xyz[first_corner], normals=normals, rgba=rgba[first_corner], labels=labels[first_corner], indices=indices.astype(np.uint32),
                stats=dict(corners=n_corners, vertices=n_vertices, max_corners_per_vertex=int(valence.max())), agree=agree)


def assert_same(im, model, what=""):
    """An IndexedMesh against the model: every array byte for byte, the counts of the stats."""
    for name in ("xyz", "normals", "rgba", "labels", "indices"):
        a, b = np.ascontiguousarray(getattr(im, name)), np.ascontiguousarray(model[name])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero((a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(axis=1))[0]
            raise AssertionError("%s: %s differs at %d of %d rows, first %d: %r vs %r" % (what, name, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]]))
    for k, v in model["stats"].items():
        assert im.stats[k] == v, (what, k, im.stats[k], v)
