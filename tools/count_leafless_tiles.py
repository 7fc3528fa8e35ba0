#!/usr/bin/env python3
"""How many 8x8 tiles of a configuration reach no leaf group, and how many reach leaf groups but no triangle?  (CPU only.)

For every tile, the kernel's own plane test (pyramid_cull_mask: nearest > 1e-3 extent + 1e-6 coarse, an all-zero box is
culled) prunes the implicit tree from the root.  Prints, per configuration, a markdown table of: root-miss tiles (the sky loop's),
leafless tiles (no child of a last-level node survives), those of them that fit the caps of a per-tile node list (listed nodes,
survivors per node, every listed node LDS resident), and the distribution of pruned-tree sizes among the leafless tiles.
Then the same tree with the triangle test behind it (pyramid_cull_tris, an all-zero slot is culled): the tiles that reach leaf
boxes split into TRIANGLE-LESS ones (every triangle of every reached group is culled) and the rest, and the triangle-less and
leafless tiles that a list of 16, 24 or 32 entries (listed nodes below the root plus reached groups) would hold.

  python tools/count_leafless_tiles.py helmet tower [--max-nodes 8] [--max-surv 4] [--size WxH]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from raytracing_c_amd import tile_classes  # noqa: E402
from raytracing_c_amd.configs import load_config  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="+")
    ap.add_argument("--max-nodes", type=int, default=8)
    ap.add_argument("--max-surv", type=int, default=4)
    ap.add_argument("--size", default=None, help="WxH instead of the configuration's")
    ap.add_argument("--margin", type=float, default=1e-3)
    a = ap.parse_args()
    for name in a.configs:
        hs, cfg = load_config(name)
        w, h, spp = cfg["width"], cfg["height"], cfg["samples"]
        if a.size:
            w, h = (int(v) for v in a.size.lower().split("x"))
        n_lds = tile_classes.lds_nodes(hs.n_nodes, hs.depth)
        c = tile_classes.classify_scene(hs, w, h, a.margin, triangles=True)
        # pixels of each tile that lie inside the image
        ty, tx = c["leafless"].shape
        px = np.minimum(8, w - 8 * np.arange(tx))[None, :] * np.minimum(8, h - 8 * np.arange(ty))[:, None]
        paths = px.astype(np.int64) * spp
        root = c["root_miss"]
        inner = c["leafless"] & ~root
        fits = inner & (c["n_listed"] <= a.max_nodes) & (c["max_surv"] <= a.max_surv) & (c["max_node"] < n_lds)
        total = int(paths.sum())
        print(f"## {name}: {w}x{h}, {spp} spp, depth {hs.depth}, {hs.n_nodes} nodes, {n_lds} in LDS (16 waves), "
              f"{ty * tx} tiles, {total / 1e6:.1f} M camera paths\n")
        print("| tiles | count | camera paths (M) | share of camera paths |")
        print("|---|---:|---:|---:|")
        for label, m in (("root-miss (sky loop today)", root), ("leafless, not root-miss", inner),
                         (f"... within the caps ({a.max_nodes} nodes, {a.max_surv} survivors, LDS)", fits),
                         ("... over the node cap", inner & (c["n_listed"] > a.max_nodes)),
                         ("... over the survivor cap", inner & (c["max_surv"] > a.max_surv)),
                         ("... a listed node outside LDS", inner & (c["max_node"] >= n_lds))):
            p = int(paths[m].sum())
            print(f"| {label} | {int(m.sum())} | {p / 1e6:.1f} | {100.0 * p / total:.1f} % |")
        print("\nPruned-tree size of the leafless tiles that are not root-miss (rows: listed nodes; columns: largest survivor "
              "count of one node):\n")
        ns = sorted(set(c["n_listed"][inner].tolist()))
        ms = sorted(set(c["max_surv"][inner].tolist()))
        print("| nodes \\ survivors | " + " | ".join(str(m) for m in ms) + " |")
        print("|---|" + "---:|" * len(ms))
        for n in ns:
            row = [int((inner & (c["n_listed"] == n) & (c["max_surv"] == m)).sum()) for m in ms]
            print(f"| {n} | " + " | ".join(str(v) for v in row) + " |")
        print()

        def line(label, m):
            p = int(paths[m].sum())
            print(f"| {label} | {int(m.sum())} | {p / 1e6:.1f} | {100.0 * p / total:.2f} % |")

        tl = c["triangleless"]
        reach = ~c["leafless"]
        print("With the triangle test behind the boxes:\n")
        print("| tiles | count | camera paths (M) | share of camera paths |")
        print("|---|---:|---:|---:|")
        line("root-miss", root)
        line("leafless, not root-miss", inner)
        line("pyramid reaches a leaf box (or a pruned tree over 64 nodes)", reach)
        line("... every triangle of every reached group is culled: triangle-less", tl)
        line("... a triangle survives", reach & ~tl)
        in_lds = (c["max_surv"] <= a.max_surv) & (c["max_node"] < n_lds)
        print("\nList size (entries: listed nodes below the root plus reached groups; survivor cap and LDS residence as above):\n")
        print("| entry cap | triangle-less tiles | camera paths (M) | leafless tiles, not root-miss | camera paths (M) |")
        print("|---:|---:|---:|---:|---:|")
        for cap in (a.max_nodes - 1, 15, 23, 31):                # a list of 8, 16, 24, 32 with the root in it
            t, l = tl & in_lds & (c["n_entries"] <= cap), inner & in_lds & (c["n_entries"] <= cap)
            print(f"| {cap + 1} | {int(t.sum())} | {paths[t].sum() / 1e6:.1f} | {int(l.sum())} | {paths[l].sum() / 1e6:.1f} |")
        if tl.any():
            q = lambda v: " / ".join(str(int(x)) for x in (np.median(v), np.percentile(v, 90), v.max()))      # noqa: E731
            print(f"\nTriangle-less tiles, median / 90th percentile / largest: listed nodes {q(c['n_listed'][tl])}, "
                  f"reached groups {q(c['n_groups'][tl])}")
        print()
        hs.free()


if __name__ == "__main__":
    main()
