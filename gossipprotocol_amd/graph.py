"""A caller-supplied network for :meth:`Ensemble.on_graph` (gp_graph; SRS v1-G).

A directed graph in CSR form: the neighbours of node i are ``indices[indptr[i]:indptr[i + 1]]`` in
the order given -- the reference's NeighbourRef array of an actor.  Self-loops are allowed,
duplicates are allowed and weight the pick, and an undirected network lists every edge both ways.
numpy only.  Whether a graph is admissible (degree >= 1 everywhere, indices below num_nodes, an LDS
image that fits) is decided by the library, not here: :func:`ensemble_graph_lds_bytes`.
"""
from __future__ import annotations

import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF
_S_TOPO = 0  # the Philox stream of Imp3D's random edge


def _philox_uniform(seed, stream, nodes, rnd, m):
    """SRS v1's U(m) for an array of node ids: Philox4x32-10 with counter (node, round, stream, 0)
    and key (seed low, seed high); floor(((y << 32) | x) * m / 2^64) of its first two words."""
    c0 = np.asarray(nodes, np.uint64) & np.uint64(_MASK)
    c1 = np.full_like(c0, rnd)
    c2 = np.full_like(c0, stream)
    c3 = np.zeros_like(c0)
    k0, k1 = seed & _MASK, (seed >> 32) & _MASK
    mask, s32 = np.uint64(_MASK), np.uint64(32)
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2  # (32 x 32 bits: no overflow in 64)
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0)) & mask, p1 & mask, ((p0 >> s32) ^ c3 ^ np.uint64(k1)) & mask, p0 & mask
    return np.array([((int(y) << 32 | int(x)) * m) >> 64 for x, y in zip(c0, c1)], np.int64)


class Graph:
    """``Graph(indptr, indices)``: the arrays as int64 / uint32 numpy arrays (copied if they are not)."""

    def __init__(self, indptr, indices):
        self.indptr = np.ascontiguousarray(indptr, np.int64)
        self.indices = np.ascontiguousarray(indices, np.uint32)
        if self.indptr.ndim != 1 or self.indices.ndim != 1 or len(self.indptr) < 1:
            raise ValueError("indptr and indices are one-dimensional, indptr has num_nodes + 1 entries")

    @property
    def num_nodes(self) -> int:
        return len(self.indptr) - 1

    @property
    def num_edges(self) -> int:
        """Entries of ``indices``: directed edges, an undirected one counts twice."""
        return len(self.indices)

    def neighbors(self, i: int):
        """nb(i), in pick order."""
        return self.indices[self.indptr[i]:self.indptr[i + 1]]

    def __repr__(self):
        return f"Graph({self.num_nodes} nodes, {self.num_edges} entries)"

    # -- constructors ---------------------------------------------------------------------------
    @classmethod
    def _from_lists(cls, lists):
        deg = np.array([len(a) for a in lists], np.int64)
        indptr = np.concatenate(([0], np.cumsum(deg)))
        flat = np.concatenate([np.asarray(a, np.int64) for a in lists]) if len(lists) and deg.sum() else np.zeros(0, np.int64)
        return cls(indptr, flat)

    @classmethod
    def from_edges(cls, n: int, edges, directed: bool = False):
        """A graph of n nodes from an (m, 2) list of (u, v) pairs.  directed: u lists v.  Otherwise u
        lists v and v lists u (a self-loop (u, u) is listed once).  A node's neighbours keep the
        order in which its edges appear in the list; an edge given twice is listed twice."""
        e = np.asarray(edges, np.int64).reshape(-1, 2)
        if len(e) and (e.min() < 0 or e.max() >= n):
            raise ValueError(f"edge endpoint outside [0, {n})")
        if directed:
            src, dst = e[:, 0], e[:, 1]
        else:
            src = np.stack([e[:, 0], e[:, 1]], 1).ravel()
            dst = np.stack([e[:, 1], e[:, 0]], 1).ravel()
            keep = np.ones(len(src), bool)
            keep[1::2] = e[:, 0] != e[:, 1]
            src, dst = src[keep], dst[keep]
        order = np.argsort(src, kind="stable")
        indptr = np.concatenate(([0], np.cumsum(np.bincount(src, minlength=n))))
        return cls(indptr, dst[order])

    @classmethod
    def ring(cls, n: int, k: int = 2):
        """A ring lattice: node i lists i - d and i + d (mod n) for d = 1 .. k / 2, in that order;
        k even, 2 <= k < n."""
        if k < 2 or k % 2 or k >= n:
            raise ValueError("ring: k must be even with 2 <= k < n")
        i = np.arange(n, dtype=np.int64)[:, None]
        d = np.arange(1, k // 2 + 1, dtype=np.int64)[None, :]
        nb = np.stack([(i - d) % n, (i + d) % n], 2).reshape(n, k)
        return cls(np.arange(n + 1, dtype=np.int64) * k, nb.ravel())

    @classmethod
    def torus(cls, w: int, h: int):
        """A 2D torus: node y * w + x lists (x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1), wrapped;
        w, h >= 2 (an edge of 2 lists its one neighbour in that direction twice)."""
        if w < 2 or h < 2:
            raise ValueError("torus: w, h >= 2")
        y, x = np.divmod(np.arange(w * h, dtype=np.int64), w)
        nb = np.stack([y * w + (x - 1) % w, y * w + (x + 1) % w, ((y - 1) % h) * w + x, ((y + 1) % h) * w + x], 1)
        return cls(np.arange(w * h + 1, dtype=np.int64) * 4, nb.ravel())

    @classmethod
    def star(cls, n: int):
        """Node 0 is the hub and lists 1 .. n - 1; every other node lists 0."""
        if n < 2:
            raise ValueError("star: n >= 2")
        return cls._from_lists([np.arange(1, n)] + [[0]] * (n - 1))

    @classmethod
    def watts_strogatz(cls, n: int, k: int, p: float, seed: int = 1):
        """A Watts-Strogatz small world, undirected and deterministic in (n, k, p, seed).

        Start from ``ring(n, k)``.  For d = 1 .. k / 2 and, inside, i = 0 .. n - 1: draw u from
        ``numpy.random.RandomState(seed).random_sample()``; if u < p and i has fewer than n - 1
        neighbours, replace the edge {i, (i + d) mod n} by {i, t}, t drawn with ``randint(n)`` until
        it is neither i nor a neighbour of i.  (RandomState is numpy's frozen legacy stream: the
        same numbers in every numpy version.)  Every node then lists its neighbours ascending."""
        if k < 2 or k % 2 or k >= n or not (0.0 <= p <= 1.0):
            raise ValueError("watts_strogatz: k even with 2 <= k < n, p in [0, 1]")
        rs = np.random.RandomState(seed)
        adj = [set() for _ in range(n)]
        for i in range(n):
            for d in range(1, k // 2 + 1):
                adj[i].add((i + d) % n)
                adj[(i + d) % n].add(i)
        for d in range(1, k // 2 + 1):
            for i in range(n):
                j = (i + d) % n
                if rs.random_sample() >= p or len(adj[i]) >= n - 1 or j not in adj[i]:
                    continue
                t = int(rs.randint(n))
                while t == i or t in adj[i]:
                    t = int(rs.randint(n))
                adj[i].remove(j)
                adj[j].remove(i)
                adj[i].add(t)
                adj[t].add(i)
        return cls._from_lists([sorted(a) for a in adj])

    @classmethod
    def lattice3d(cls, g: int):
        """The reference's 3D topology as a graph: node i * g^2 + j * g + k lists, where they exist,
        (i-1), (i+1), (j+1), (j-1), (k+1), (k-1) -- the slot order of its neighbour arrays
         -- so a graph run draws what the built-in "3D" kernels draw."""
        return cls._from_lists(cls._lattice_lists(g))

    @classmethod
    def imp3d(cls, g: int, seed: int):
        """:meth:`lattice3d` plus, as every node's last slot, the random edge the built-in "Imp3D"
        topology draws for this seed: U_TOPO(P - 1), the stream-0 Philox draw of the node."""
        lists = cls._lattice_lists(g)
        P = g ** 3
        rnd = _philox_uniform(int(seed), _S_TOPO, np.arange(P), 0, P - 1)
        return cls._from_lists([a + [int(r)] for a, r in zip(lists, rnd)])

    @staticmethod
    def _lattice_lists(g):
        if g < 2:
            raise ValueError("lattice: g >= 2")
        g2, out = g * g, []
        for i in range(g):
            for j in range(g):
                for k in range(g):
                    idx, a = i * g2 + j * g + k, []
                    if i - 1 >= 0:
                        a.append(idx - g2)
                    if i + 1 < g:
                        a.append(idx + g2)
                    if j + 1 < g:
                        a.append(idx + g)
                    if j - 1 >= 0:
                        a.append(idx - g)
                    if k + 1 < g:
                        a.append(idx + 1)
                    if k - 1 >= 0:
                        a.append(idx - 1)
                    out.append(a)
        return out
