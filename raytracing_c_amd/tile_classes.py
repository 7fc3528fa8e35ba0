"""Host model of the path kernel's per-tile pyramid test (rt_tile.hip.h: tile_pyramid, the path kernel's tile_root_miss; rt_dev.hip.h: pyramid_cull_mask).

For every 8x8 tile of a frame: the four side planes of the pyramid through the tile's pixel footprint, and the implicit 8-ary
tree pruned by them, breadth-first from the root.  A tile is ROOT-MISS when the pyramid misses every child box of the root
(the kernel's sky tiles) and LEAFLESS when the pruned tree holds no child of a last-level node: no camera ray of the tile that
is NaN-free reaches a leaf group.  Given the scene's triangles, a tile that does reach leaf groups is TRIANGLE-LESS when the
pyramid's triangle test (pyramid_cull_tris) culls every triangle of every group it reaches: its camera rays enter leaf boxes and
accept nothing.  fp32 throughout, without the kernel's fused multiply-adds: a count and a test oracle (with a
stricter margin), not a bit-exact replay.
"""
import numpy as np

F = np.float32


def lds_nodes(n_nodes, depth, wg_waves=16):
    """Nodes [0, n) the path kernel keeps in LDS (rt_launch.cpp: lds_split with the constants of rt_device.h)."""
    per_wave = max(depth, 1) * 256 + 1536
    room = (160 * 1024 - 64 - wg_waves * per_wave) // 208
    return min(n_nodes, max(room, 0))


def tile_pyramids(cam_rows, focal_length, width, height):
    """(tiles_y, tiles_x, 4, 3) outward plane normals and the (3,) ray origin, as the kernel's tile set-up computes them."""
    cam = np.asarray(cam_rows, F).reshape(-1, 4)[:3]
    ty, tx = (height + 7) // 8, (width + 7) // 8
    inv_w, inv_h, asp = F(1.0) / F(width), F(1.0) / F(height), F(width) / F(height)
    m = F(0.05)
    x0 = (np.arange(tx, dtype=F) * F(8))[None, :]
    y0 = (np.arange(ty, dtype=F) * F(8))[:, None]
    ux0 = (x0 - F(0.5) - m) * F(2.0) * inv_w - F(1.0)
    ux1 = (x0 + F(7.5) + m) * F(2.0) * inv_w - F(1.0)
    uy0 = (y0 - F(0.5) - m) * F(2.0) * inv_h - F(1.0)
    uy1 = (y0 + F(7.5) + m) * F(2.0) * inv_h - F(1.0)
    c = np.zeros((ty, tx, 4, 3), F)
    for q in range(4):
        cx = np.broadcast_to((ux1 if q in (1, 2) else ux0) * asp, (ty, tx))
        cy = np.broadcast_to(-(uy1 if q >= 2 else uy0), (ty, tx))
        cz = F(-focal_length)
        for i in range(3):
            c[:, :, q, i] = cam[i, 0] * cx + cam[i, 1] * cy + cam[i, 2] * cz
    pn = np.zeros((ty, tx, 4, 3), F)
    for q in range(4):
        n = np.cross(c[:, :, q], c[:, :, (q + 1) & 3]).astype(F)
        flip = np.sum(n * c[:, :, (q + 2) & 3], axis=-1) > 0
        n[flip] = -n[flip]
        pn[:, :, q] = n
    return pn, cam[:, 3].copy()


def cull_masks(nodes, node_idx, pn, origin, margin=1e-3):
    """pyramid_cull_mask for pairs (node_idx[i], pn[i]): (n, 8) bool, True = no ray inside the pyramid enters the child."""
    nb = nodes[node_idx]                                      # (n, 6, 8): min x y z, max x y z
    mn, mx = nb[:, 0:3, :], nb[:, 3:6, :]
    o = origin.astype(F)[None, :, None]
    empty = np.all(nb == 0, axis=1)
    nrm = pn[:, :, :, None]                                   # (n, 4 planes, 3 axes, 1)
    lo = nrm * (mn - o)[:, None]                              # (n, 4, 3, 8)
    hi = nrm * (mx - o)[:, None]
    nearest = np.minimum(lo, hi).sum(axis=2, dtype=F)
    extent = np.maximum(np.abs(lo), np.abs(hi)).sum(axis=2, dtype=F)
    coarse = (np.abs(nrm) * (np.abs(o)[:, None] + np.maximum(np.abs(mn), np.abs(mx))[:, None])).sum(axis=2, dtype=F)
    with np.errstate(invalid="ignore"):
        outside = nearest > F(margin) * extent + F(1e-6) * coarse
    return empty | outside.any(axis=1)


def cull_tris(soa, group, pn, origin, margin=1e-3, zero_culled=True):
    """pyramid_cull_tris for pairs (group[i], pn[i]): (n, 8) bool, True = the fattened triangle lies outside one plane.  soa: the
    (9, slots) triangle block (x0 x1 x2 y0 y1 y2 z0 z1 z2; slot 8 g + k is triangle k of group g), from which the device keeps a
    vertex and two edges.  zero_culled: an all-zero slot -- the padding of a partly filled group -- counts as culled whatever the
    planes say (leafless_walk: such a triangle is never accepted)."""
    soa = np.asarray(soa, F)
    n_groups = soa.shape[1] // 8
    inside = np.asarray(group) < n_groups
    slots = np.where(inside, group, 0)[:, None] * 8 + np.arange(8)[None, :]          # (n, 8)
    v = soa[:, slots] * inside[None, :, None].astype(F)                               # (9, n, 8); a group past the block: zeros
    a = np.stack([v[0], v[3], v[6]], axis=1)                                          # (n, 3 axes, 8)
    e1 = np.stack([v[1], v[4], v[7]], axis=1) - a
    e2 = np.stack([v[2], v[5], v[8]], axis=1) - a
    zero = np.all(v == 0, axis=0)
    o = origin.astype(F)[None, None, :, None]
    nrm = pn[:, :, :, None]                                                           # (n, 4 planes, 3 axes, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        band = F(2.5e-4) * (np.abs((nrm * e1[:, None]).sum(axis=2, dtype=F)) + np.abs((nrm * e2[:, None]).sum(axis=2, dtype=F)))
        outside = np.ones(band.shape, bool)                                           # (n, 4, 8)
        for vert in (a, a + e1, a + e2):
            vert = vert[:, None]                                                      # (n, 1, 3, 8)
            p = nrm * (vert - o)
            val = p.sum(axis=2, dtype=F)
            extent = np.abs(p).sum(axis=2, dtype=F)
            coarse = (np.abs(nrm) * (np.abs(o) + np.abs(vert))).sum(axis=2, dtype=F)
            outside &= val - band > F(margin) * extent + F(1e-6) * coarse
    culled = outside.any(axis=1)
    return culled | zero if zero_culled else culled


def _cull_chunked(nodes, node, pn, origin, margin, chunk=1 << 17):
    out = np.empty((len(node), 8), bool)
    for a in range(0, len(node), chunk):
        out[a:a + chunk] = cull_masks(nodes, node[a:a + chunk], pn[a:a + chunk], origin, margin)
    return out


def classify_tiles(nodes, depth, cam_rows, focal_length, width, height, margin=1e-3, give_up=64, tris=None, zero_culled=True):
    """Prune the tree per tile.  Returns a dict of (tiles_y, tiles_x) arrays:
    root_miss, leafless (root-miss tiles included), n_listed (nodes of the pruned tree, the root counts), max_surv (largest
    number of surviving children of one listed node), max_node (largest listed node index).  A tile whose pruned tree grows
    past `give_up` nodes is not followed further and counts as not leafless (far over any list the kernel would keep).
    With `tris`, the triangle block in soa_array() form, also: triangleless (the pyramid reaches leaf groups, and cull_tris culls
    every triangle of each of them; never a leafless tile), n_groups (leaf groups reached) and n_entries (listed nodes below the
    root plus reached groups: what the kernel's per-tile list would hold)."""
    nodes = np.asarray(nodes, F).reshape(-1, 6, 8)
    pn, origin = tile_pyramids(cam_rows, focal_length, width, height)
    ty, tx = pn.shape[:2]
    n_tiles = ty * tx
    pn = pn.reshape(n_tiles, 4, 3)
    leaf_level = depth - 1
    reached_leaf = np.zeros(n_tiles, bool)
    n_listed = np.zeros(n_tiles, np.int64)
    max_surv = np.zeros(n_tiles, np.int64)
    max_node = np.zeros(n_tiles, np.int64)
    root_miss = np.zeros(n_tiles, bool)
    n_groups = np.zeros(n_tiles, np.int64)
    has_tri = np.zeros(n_tiles, bool)
    leaf0 = (8 ** max(depth, 0) - 1) // 7                     # index of leaf group 0 in the implicit numbering of the tree
    if leaf_level < 0 or len(nodes) == 0:
        reached_leaf[:] = True
    else:
        tile = np.arange(n_tiles)
        node = np.zeros(n_tiles, np.int64)
        for level in range(leaf_level + 1):
            if len(tile) == 0:
                break
            surv = ~_cull_chunked(nodes, node, pn[tile], origin, margin)       # (n, 8)
            ns = surv.sum(axis=1)
            np.add.at(n_listed, tile, 1)
            np.maximum.at(max_surv, tile, ns)
            np.maximum.at(max_node, tile, node)
            if level == 0:
                root_miss = ns == 0
            if level == leaf_level:
                reached_leaf[tile[ns > 0]] = True
                if tris is not None:
                    pi, k = np.nonzero(surv)
                    np.add.at(n_groups, tile[pi], 1)
                    group = 8 * node[pi] + 1 + k - leaf0
                    for a in range(0, len(pi), 1 << 15):
                        b = slice(a, a + (1 << 15))
                        kept = ~cull_tris(tris, group[b], pn[tile[pi[b]]], origin, margin, zero_culled)
                        has_tri[tile[pi[b]][kept.any(axis=1)]] = True
                break
            pi, k = np.nonzero(surv)
            tile, node = tile[pi], 8 * node[pi] + 1 + k
            reached_leaf[n_listed + np.bincount(tile, minlength=n_tiles) > give_up] = True
            keep = ~reached_leaf[tile]
            tile, node = tile[keep], node[keep]
    shape = (ty, tx)
    out = dict(root_miss=root_miss.reshape(shape), leafless=(~reached_leaf).reshape(shape), n_listed=n_listed.reshape(shape),
               max_surv=max_surv.reshape(shape), max_node=max_node.reshape(shape))
    if tris is not None:
        out.update(triangleless=((n_groups > 0) & ~has_tri).reshape(shape), n_groups=n_groups.reshape(shape),
                   n_entries=(n_listed - 1 + n_groups).reshape(shape))
    return out


def classify_scene(hs, width, height, margin=1e-3, triangles=False, zero_culled=True):
    cam = hs.scene.camera
    rows = [[cam.view_matrix.rows[i][j] for j in range(4)] for i in range(4)]
    return classify_tiles(hs.nodes_array(), hs.depth, rows, cam.focal_length, width, height, margin,
                          tris=hs.soa_array() if triangles else None, zero_culled=zero_culled)
