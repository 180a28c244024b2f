"""The --mask option of tools/query_nearest_bench.py, query_hits_bench.py and query_sweep_bench.py: what the filtered walk queries
(Renderer.query_* with mask=..., set_object_masks) cost next to today's call.

  none   today's call (mask=None): the unfiltered kernel instantiation
  ones   the filtered instantiation with nothing hidden: no table, the scalar row mask 0xFFFFFFFF
  half   a table that hides the instances of odd index (mask 0; every other object all ones), scalar row mask 0xFFFFFFFF.  The bench
         scene (host.atrium_scene) is ONE instance: there this hides nothing and measures the table's loads alone
  rows   a table of one bit per object, 1 << (index % 4), and a device tensor of per-row masks drawn from {1, 3, 7, all ones}: every row
         sees the objects of bit 0 (the whole bench scene), so the work is the unfiltered call's plus the mask loads
"""
MODES = ("none", "ones", "half", "rows")
ONES = 0xFFFFFFFF


def add_argument(ap):
    ap.add_argument("--mask", choices=MODES, default="none", help="filtered queries: " + ", ".join(MODES) + " (see tools/query_masks.py)")


def setup(r, sc, mode, n, seed=2026):
    """Sets the context's object masks for `mode` and returns the queries' mask keyword: None, an int, or an int32 device tensor (n,)."""
    import numpy as np
    import torch
    m = len(sc.instances) + len(sc.spheres) + len(sc.planes)
    if mode == "none":
        return None
    if mode == "ones":
        r.set_object_masks(None)
        return ONES
    if mode == "half":
        table = np.full(m, ONES, np.uint32)
        table[1:len(sc.instances):2] = 0
        r.set_object_masks(table)
        return ONES
    r.set_object_masks((1 << (np.arange(m) % 4)).astype(np.uint32))
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.choice(np.array([1, 3, 7, ONES], np.uint32), n).view(np.int32)).cuda()
