"""The definition of init_method "skeleton_device" (the header comment of p3_skeleton_from_seg) restated on the host: torch on the CPU
for the edge mask, scipy.ndimage for the closing, numpy for Zhang-Suen, plain loops for the graph and the paths.  Written to the definition, step by step and
under its step numbers; the product never imports it.  Shared by test_skeleton_thin_cpu.py and test_skeleton_thin_gpu.py."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.ndimage as ndi
import torch

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], dtype=bool)
DIRS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))          # raster order: ascending neighbour id


def edge_mask(seg, level):
    """step 1: seg [C, H, W] fp32 torch -> bool [H, W] numpy"""
    m = (level < seg[0]).float()
    p = torch.nn.functional.pad(m[None, None], (1, 1, 1, 1), mode="replicate")[0, 0]
    gx = ((p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])) / 8
    gy = ((p[2:, :-2] - p[:-2, :-2]) + 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])) / 8
    g = torch.sqrt((2 * gx) ** 2 + (2 * gy) ** 2)
    if seg.shape[0] >= 2:
        g = torch.clamp(seg[1] + g, 0, 1)
    return (level < g).numpy()


def closing(edge):
    """steps 2 and 3: bool [H, W] -> the closed working image, bool [H+4, W+4]"""
    work = np.pad(edge, 2, mode="edge")
    return ndi.binary_erosion(ndi.binary_dilation(work, structure=CROSS, border_value=0), structure=CROSS, border_value=1)


def thin(image):
    """step 4: Zhang-Suen.  -> (skeleton, rounds): the last round, which deletes nothing, is counted"""
    img = image.astype(np.uint8).copy()
    rounds = 0
    while True:
        gone = False
        for sub in (1, 2):
            q = np.pad(img, 1)
            P2, P3, P4, P5 = q[:-2, 1:-1], q[:-2, 2:], q[1:-1, 2:], q[2:, 2:]
            P6, P7, P8, P9 = q[2:, 1:-1], q[2:, :-2], q[1:-1, :-2], q[:-2, :-2]
            seq = (P2, P3, P4, P5, P6, P7, P8, P9, P2)
            B = sum(s.astype(np.int32) for s in seq[:-1])
            A = sum(((a == 0) & (b == 1)).astype(np.int32) for a, b in zip(seq[:-1], seq[1:]))
            cond = (P2 * P4 * P6 == 0) & (P4 * P6 * P8 == 0) if sub == 1 else (P2 * P4 * P8 == 0) & (P2 * P6 * P8 == 0)
            delete = (img == 1) & (2 <= B) & (B <= 6) & (A == 1) & cond
            gone = gone or bool(delete.any())
            img = np.where(delete, 0, img).astype(np.uint8)
        rounds += 1
        if not gone:
            return img.astype(bool), rounds


def links_of(sk):
    """step 6 for one image: bool [H, W] -> (pixels [n, 2] of the nodes in raster order, sorted list of links (i, j) with i < j, node ids local)"""
    H, W = sk.shape
    q = np.pad(sk, 1)
    on = lambda r, c: bool(q[r + 1, c + 1])
    pix = [(int(r), int(c)) for r, c in zip(*np.nonzero(sk))]
    nbrs = {}
    for r, c in pix:
        mine = []
        for dr, dc in DIRS:
            if not on(r + dr, c + dc):
                continue
            if dr != 0 and dc != 0 and (on(r + dr, c) or on(r, c + dc)):
                continue
            mine.append((r + dr, c + dc))
        if mine:
            nbrs[(r, c)] = mine
    nodes = [p for p in pix if p in nbrs]
    ident = {p: i for i, p in enumerate(nodes)}
    links = sorted({(min(ident[p], ident[o]), max(ident[p], ident[o])) for p in nodes for o in nbrs[p]})
    return np.array(nodes, dtype=np.int64).reshape(-1, 2), links


def paths_of(n, links):
    """step 7 for one image: -> list of paths (lists of local node ids), ordered by (first node, second node)"""
    adj = [[] for _ in range(n)]
    for i, j in links:
        adj[i].append(j)
        adj[j].append(i)
    adj = [sorted(a) for a in adj]
    deg = [len(a) for a in adj]
    paths, on_chain = [], set()
    for u in range(n):
        if deg[u] == 2:
            continue
        for a in adj[u]:
            chain = [u, a]
            while deg[chain[-1]] == 2:
                x, y = adj[chain[-1]]
                chain.append(y if x == chain[-2] else x)
            on_chain.update(chain)
            if (chain[0], chain[1]) < (chain[-1], chain[-2]):
                paths.append(chain)
    for u in range(n):          # ascending: the first node of a cycle met is its smallest
        if deg[u] != 2 or u in on_chain:
            continue
        cycle = [u, adj[u][0]]
        while cycle[-1] != u:
            x, y = adj[cycle[-1]]
            cycle.append(y if x == cycle[-2] else x)
        on_chain.update(cycle)
        paths.append(cycle)
    return sorted(paths, key=lambda p: (p[0], p[1]))


def stages(seg, level):
    """one image, every intermediate: edge, closed (working frame), skeleton (H x W, before the link-less pixels go), rounds, nodes, links, paths"""
    edge = edge_mask(seg, level)
    closed = closing(edge)
    thinned, rounds = thin(closed)
    skeleton = thinned[2:-2, 2:-2]
    nodes, links = links_of(skeleton)
    return SimpleNamespace(edge=edge, closed=closed, thinned=thinned, skeleton=skeleton, rounds=rounds, nodes=nodes, links=links, paths=paths_of(len(nodes), links))


def container(seg_batch, level):
    """step 8: seg [B, C, H, W] fp32 torch (host) -> the container as host tensors, counts, the per-image stages"""
    per = [stages(s, level) for s in seg_batch]
    pos, degrees, path_index, path_delim, batch, batch_delim = [], [], [], [0], [], [0]
    n0, longest = 0, 0
    for b, st in enumerate(per):
        n = len(st.nodes)
        deg = np.bincount(np.array(st.links, dtype=np.int64).reshape(-1), minlength=n) if n else np.zeros(0, dtype=np.int64)
        pos.append(st.nodes.astype(np.float32))
        degrees.append(deg.astype(np.int64))
        batch.append(np.full(n, b, dtype=np.int64))
        for p in st.paths:
            path_index.extend(v + n0 for v in p)
            path_delim.append(len(path_index))
            longest = max(longest, len(p) - (1 if p[0] == p[-1] else 0))
        batch_delim.append(len(path_delim) - 1)
        n0 += n
    i64 = lambda v: torch.tensor(np.asarray(v, dtype=np.int64).reshape(-1), dtype=torch.int64)
    out = SimpleNamespace(pos=torch.tensor(np.concatenate(pos).reshape(-1, 2), dtype=torch.float32), degrees=i64(np.concatenate(degrees)), path_index=i64(path_index),
                          path_delim=i64(path_delim), batch=i64(np.concatenate(batch)), batch_delim=i64(batch_delim), batch_size=len(per), stages=per)
    out.counts = (n0, len(path_index), len(path_delim) - 1, longest)
    return out


@functools.lru_cache(maxsize=None)
def container_of(name):
    """the container of a named scene or batch of tests/skeleton_thin_cases.py, computed once and shared: do not modify"""
    from tests import skeleton_thin_cases as K
    return container(K.seg_of(name), K.LEVEL)
