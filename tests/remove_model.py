"""NumPy yardstick of block removal, written from the contract.

The removed SET: from the block list, or — for the distance entry — the float32 rule restated operation by operation
    block_size = voxel_size * (float)vps;  o_k = (float)b_k * block_size;  d_k = o_k - center_k;
    d2 = (dx * dx + dy * dy) + dz * dz;  removed iff d2 > max_distance * max_distance.
The expected MAP is the blocks downloaded before the call minus that set.  For the stored products the yardstick is
equivalence with a second, fresh context that was only ever given the kept blocks (tests/remove_case.py); what this file adds for
them are the tile lists the locality cases judge with: which blocks a mesh refresh has to re-mesh, which tiles an ESDF refresh has
to recompute."""
import numpy as np

f32 = np.float32


def distant_f32(blocks, center, max_distance, voxel_size, vps):
    """(n,) bool: the rule, every operation in float32 and in the order of the contract."""
    b = np.asarray(blocks, np.int64).reshape(-1, 3)
    c = np.asarray(center, f32).reshape(3)
    block_size = f32(voxel_size) * f32(vps)
    o = b.astype(f32) * block_size
    d = o - c[None, :]
    sq = d * d
    d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    m = f32(max_distance)
    assert o.dtype == d.dtype == sq.dtype == d2.dtype == np.float32
    return d2 > m * m


def distance_f64(blocks, center, voxel_size, vps):
    """(n,) f64: the distance of every block's ORIGIN from the centre, from the f32 inputs the device gets."""
    b = np.asarray(blocks, np.int64).reshape(-1, 3).astype(np.float64)
    c = np.asarray(center, f32).reshape(3).astype(np.float64)
    return np.linalg.norm(b * (float(f32(voxel_size)) * float(vps)) - c[None, :], axis=1)


def assert_away_from_threshold(blocks, center, max_distance, voxel_size, vps, margin=1e-3):
    """No block within `margin` metres of the threshold: there the f32 rule and an f64 evaluation must agree, so no GPU run depends on
    how a borderline block rounds.  (f32 carries 24 bits: at block origins of a few metres the rule's d2 is good to ~1e-6 m^2.)"""
    dist = distance_f64(blocks, center, voxel_size, vps)
    gap = np.abs(dist - float(f32(max_distance)))
    assert len(dist) == 0 or gap.min() > margin, (float(gap.min()), margin)
    far64 = dist > float(f32(max_distance))
    far32 = distant_f32(blocks, center, max_distance, voxel_size, vps)
    assert (far64 == far32).all()
    return far32


def _rows(a):
    return [tuple(int(v) for v in r) for r in np.asarray(a).reshape(-1, 3)]


def removed_of_list(resident, listed):
    """The blocks a list call removes: the listed ones that are resident, once each, ascending by (x, y, z)."""
    res = set(_rows(resident))
    return np.array(sorted(set(_rows(listed)) & res), np.int32).reshape(-1, 3)


def removed_of_distance(resident, center, max_distance, voxel_size, vps):
    res = np.array(sorted(_rows(resident)), np.int32).reshape(-1, 3)
    return res[distant_f32(res, center, max_distance, voxel_size, vps)].reshape(-1, 3)


def kept_of(idx, removed, *arrays):
    """The rows of idx (and of the arrays that go with it) whose block is not in `removed`."""
    gone = set(_rows(removed))
    keep = np.array([r not in gone for r in _rows(idx)], bool)
    return (np.asarray(idx)[keep].reshape(-1, 3),) + tuple(a[keep] for a in arrays)


# ---- slots: what the compaction has to do ---------------------------------------------------------------------------------------
def moves_needed(keep):
    """keep: (nt,) bool by slot.  Returns (nt', moves): every kept tile at a slot >= nt' needs one of the removed slots < nt'."""
    keep = np.asarray(keep, bool)
    nt2 = int(keep.sum())
    return nt2, int(keep[nt2:].sum())


# ---- the tile lists of the locality cases -----------------------------------------------------------------------------------------
def mesh_blocks_to_remesh(kept_blocks, removed_blocks, stale_blocks=()):
    """The kept blocks a refresh re-meshes: those with a stale tile, and — for stale and removed blocks alike — the up to seven
    blocks at -x / -y / -z offsets whose border cubes read them."""
    kept = set(_rows(kept_blocks))
    out = set()
    for b in _rows(removed_blocks) + _rows(np.asarray(stale_blocks, np.int64).reshape(-1, 3)):
        for o in range(8):
            n = (b[0] - (o & 1), b[1] - ((o >> 1) & 1), b[2] - (o >> 2))
            if n in kept:
                out.add(n)
    return sorted(out)


def esdf_tiles_to_recompute(kept_tiles, removed_tiles, grow):
    """The kept tiles within `grow` tiles of a removed one on every axis."""
    kept, gone = np.asarray(kept_tiles, np.int64).reshape(-1, 3), np.asarray(removed_tiles, np.int64).reshape(-1, 3)
    if not len(gone) or not len(kept):
        return kept[:0]
    near = (np.abs(kept[:, None, :] - gone[None, :, :]).max(axis=2) <= grow).any(axis=1)
    return kept[near]
