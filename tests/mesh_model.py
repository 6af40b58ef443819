"""The yardstick of the mesh tests: a NumPy restatement of the mesh contract (DESIGN.md, section "Semantic mesh"), written
from the contract and not from the kernels.  Operands are np.float32 throughout (IEEE single, no fused operations).

    mesh_from_blocks(indices, tsdf, vps, voxel_size, min_weight, labels) -> dict(blocks, xyz, normals, rgba, labels, degenerate)

takes host-layout blocks as HipIntegrator.download() returns them (indices ascending by (x, y, z), one row of vps^3 voxels per
block in x + vps * (y + vps * z) order) and produces the ordered vertex arrays.  One vectorised pass per block.
The triangle table comes from the library's single data file (kimera_semantics_amd.mesh.load_tri_table)."""
import numpy as np

from kimera_semantics_amd.mesh import EDGE_CORNERS, load_tri_table

F = np.float32
BLOCK_DTYPE = np.dtype([("block", "<i4", (3,)), ("first_vertex", "<u4"), ("n_vertices", "<u4")])


def corner_offset(i):
    return np.array([i & 1, (i >> 1) & 1, (i >> 2) & 1])


def _halo(bi, lookup, field, vps, fill):
    """(vps+1)^3 array [z, y, x] of `field[block][voxel]` over the block and its +x / +y / +z neighbours."""
    out = np.full((vps + 1,) * 3, fill, dtype=field.dtype)
    for o in range(8):
        dx, dy, dz = o & 1, (o >> 1) & 1, o >> 2
        j = lookup.get((bi[0] + dx, bi[1] + dy, bi[2] + dz))
        if j is None:
            continue
        g = field[j].reshape(vps, vps, vps)
        sx = slice(0, vps) if not dx else slice(vps, vps + 1)
        sy = slice(0, vps) if not dy else slice(vps, vps + 1)
        sz = slice(0, vps) if not dz else slice(vps, vps + 1)
        gx = slice(0, vps) if not dx else slice(0, 1)
        gy = slice(0, vps) if not dy else slice(0, 1)
        gz = slice(0, vps) if not dz else slice(0, 1)
        out[sz, sy, sx] = g[gz, gy, gx]
    return out


def mesh_from_blocks(indices, tsdf, vps, voxel_size, min_weight=1e-4, labels=None, table=None):
    indices = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
    table = load_tri_table() if table is None else table
    vs, mw = F(voxel_size), F(min_weight)
    dist = np.ascontiguousarray(tsdf["distance"], dtype=F)
    wgt = np.ascontiguousarray(tsdf["weight"], dtype=F)
    col = np.ascontiguousarray(tsdf["color"]).view("<u4").reshape(len(indices), -1)
    lab = np.zeros(dist.shape, np.uint8) if labels is None else np.ascontiguousarray(labels, dtype=np.uint8)
    order = np.lexsort((indices[:, 2], indices[:, 1], indices[:, 0]))
    lookup = {tuple(int(v) for v in indices[j]): j for j in range(len(indices))}
    out = dict(xyz=[], normals=[], rgba=[], labels=[])
    blocks, n_deg, first = [], 0, 0
    tri = np.asarray(table)[:, :15].reshape(256, 5, 3)   # (the sixteenth entry is the terminator)
    tri_n = (tri[:, :, 0] >= 0).sum(axis=1)
    for j in order:
        bi = tuple(int(v) for v in indices[j])
        d, w = _halo(bi, lookup, dist, vps, F(0)), _halo(bi, lookup, wgt, vps, F(0))
        ok = np.ones((vps,) * 3, bool)
        case = np.zeros((vps,) * 3, np.int64)
        for i in range(8):
            ox, oy, oz = corner_offset(i)
            sl = (slice(oz, oz + vps), slice(oy, oy + vps), slice(ox, ox + vps))
            ok &= w[sl] >= mw
            case |= (d[sl] < F(0)).astype(np.int64) << i
        sel = ok & (tri_n[case] > 0)
        cz, cy, cx = np.nonzero(sel)            # ascending z, y, x = ascending linear index
        if len(cx) == 0:
            continue
        c, l = _halo(bi, lookup, col, vps, np.uint32(0)), _halo(bi, lookup, lab, vps, np.uint8(0))
        cs = case[cz, cy, cx]
        # one row per (cube, triangle slot), cube-major
        nt = tri_n[cs]
        cube = np.repeat(np.arange(len(cs)), nt)
        slot = np.concatenate([np.arange(n) for n in nt])
        edges = tri[cs[cube], slot].astype(np.int64)   # (T, 3)
        ea = np.array([a for a, _ in EDGE_CORNERS])[edges]
        eb = np.array([b for _, b in EDGE_CORNERS])[edges]
        base = np.stack([cx[cube], cy[cube], cz[cube]], axis=1)[:, None, :]           # (T, 1, 3) local voxel of the cube
        offs = np.array([corner_offset(i) for i in range(8)])
        la, lb = base + offs[ea], base + offs[eb]                                     # (T, 3, 3) local corner voxels
        da, db = d[la[..., 2], la[..., 1], la[..., 0]], d[lb[..., 2], lb[..., 1], lb[..., 0]]
        org = np.array(bi, dtype=np.int64) * vps
        pa = ((la + org).astype(F) + F(0.5)) * vs
        pb = ((lb + org).astype(F) + F(0.5)) * vs
        t = da / (da - db)
        p = pa + t[..., None] * (pb - pa)
        assert p.dtype == F and t.dtype == F
        own = np.where((t < F(0.5))[..., None], la, lb)
        u, v = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        cr = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        ln = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
        keep = ln != F(0)
        n_deg += int((~keep).sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            nrm = cr / ln[:, None]
        p, nrm, own = p[keep], nrm[keep], own[keep]
        nv = 3 * len(p)
        if nv == 0:
            continue
        out["xyz"].append(p.reshape(-1, 3))
        out["normals"].append(np.repeat(nrm, 3, axis=0))
        o = own.reshape(-1, 3)
        out["rgba"].append(c[o[:, 2], o[:, 1], o[:, 0]])
        out["labels"].append(l[o[:, 2], o[:, 1], o[:, 0]])
        blocks.append((bi, first, nv))
        first += nv
    res = dict(degenerate=n_deg)
    res["blocks"] = np.array(blocks, dtype=BLOCK_DTYPE) if blocks else np.zeros(0, BLOCK_DTYPE)
    res["xyz"] = np.concatenate(out["xyz"]).astype(F) if blocks else np.zeros((0, 3), F)
    res["normals"] = np.concatenate(out["normals"]).astype(F) if blocks else np.zeros((0, 3), F)
    rg = np.concatenate(out["rgba"]).astype("<u4") if blocks else np.zeros(0, "<u4")
    res["rgba"] = rg.view(np.uint8).reshape(-1, 4)
    res["labels"] = np.concatenate(out["labels"]).astype(np.uint8) if blocks else np.zeros(0, np.uint8)
    return res


def model_of(integrator, min_weight=1e-4):
    """The model's mesh of the map an integrator holds (through download())."""
    idx, t, s = integrator.download()
    return mesh_from_blocks(idx, t, integrator.vps, integrator.cfg.voxel_size, min_weight, labels=s["label"])


def assert_same(mesh, model, what=""):
    """Every array bit for bit, same order."""
    assert len(mesh.xyz) == len(model["xyz"]), (what, len(mesh.xyz), len(model["xyz"]))
    assert mesh.blocks.tobytes() == model["blocks"].astype(mesh.blocks.dtype).tobytes(), what
    for name in ("xyz", "normals", "rgba", "labels"):
        a, b = np.ascontiguousarray(getattr(mesh, name)), np.ascontiguousarray(model[name])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero((a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(axis=1))[0]
            raise AssertionError("%s: %s differs at %d of %d vertices, first %d: %r vs %r" % (what, name, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]]))
