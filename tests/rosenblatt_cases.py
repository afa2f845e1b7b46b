"""The cases test_rosenblatt_cpu.py and test_gpu_rosenblatt.py share: sample_ref.CASES with sample_real_ref.case's nodes, non-negative
and signed, and the two trains test_gpu_sample_sq_real.py adds, restated with its seeds: edge_ranks (sample_sq_ref's train with the
bonds 4, 5, 15, 16 and a mode of one node) and tile_edges (modes of 2, 15, 16, 17, 31 and 32 nodes, bonds 4, 5, 16, 17).  Together
they carry the ranks 1, 3, 4, 5, 15, 16, 17, 64, 65 and 128 and modes of 1, 2, 15, 16, 17, 31, 32, 64, 65, 130 and 1025 nodes."""
import functools

import numpy as np

import sample_ref as S
import sample_sq_real_ref as Q
import sample_sq_ref as SQ

ALL = [(k, s) for k in S.CASES for s in (False, True)] + [("edge_ranks", True), ("tile_edges", True)]
IDS = [k + ("_signed" if s else "") for k, s in ALL]
TILE_EDGES = ([2, 15, 16, 17, 31, 32], [1, 4, 5, 16, 17, 3, 1])
NPTS = 500                                          # of a case's 2000 uniforms


def _nodes(n, seed):
    rng = np.random.default_rng(seed)
    return [np.cumsum(rng.uniform(0.2, 1.0, nk)) - rng.uniform(0.0, 3.0) for nk in n]


@functools.lru_cache(maxsize=None)
def case(name, signed):
    """(cores, u [NPTS][d], nodes); shared, not to be modified"""
    if name == "edge_ranks":
        cores, u, _ = SQ.edge_case()
        nodes = _nodes(SQ.EDGE_RANKS[0], 4517)
    elif name == "tile_edges":
        n, r = TILE_EDGES
        rng = np.random.default_rng(1516)
        cores, u, nodes = [rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(len(n))], rng.random((S.NPTS, len(n))), _nodes(n, 1517)
    else:
        cores, u, nodes = Q.case(name, signed)
    u = np.ascontiguousarray(u[:NPTS])
    u.setflags(write=False)
    return cores, u, nodes


def cloud(nodes, npts, seed):
    """seeded uniform points in the box of the nodes"""
    rng = np.random.default_rng(seed)
    return np.stack([np.clip(t[0] + (t[-1] - t[0]) * rng.random(npts), t[0], t[-1]) if t.size > 1 else np.full(npts, t[0]) for t in nodes], axis=1)
