"""Blast radius of the ranked root causes as the device computed it (include/krca.h g1,
csrc/graph_reach.hip): which nodes each of up to 64 sources reaches, how many hops
away, how many of them are marked (anomalous), and the greedy cover of the marked nodes by the radii.

:class:`BlastRadius` holds the arrays of krca_graph_reach / krca_graph_reach_cover as host numpy
arrays; its walkers are host code over those arrays (they need no GPU and are tested on restated
arrays).  ``NativeEngine.blast_radius`` builds it.
"""
from dataclasses import dataclass

import numpy as np

DIRECTIONS = {"dependents": 0, "dependencies": 1}  # KRCA_REACH_DEPENDENTS / KRCA_REACH_DEPENDENCIES


@dataclass
class BlastRadius:
    reach: np.ndarray                # uint64 [N]: bit k = source k reaches the node (the source itself included)
    hist: np.ndarray                 # int64 [K][H]: nodes at h hops from source k; the last bin is "H - 1 or more"
    hist_marked: np.ndarray          # int64 [K][H]: the same over the marked nodes
    depth: np.ndarray                # int32 [K]: the largest hop count source k reaches
    order: np.ndarray = None         # int32 [K] (cover=True): greedy picks, -1 past the last
    gain: np.ndarray = None          # int64 [K]: marked nodes each pick added, 0 past the last
    exclusive: np.ndarray = None     # int64 [K]: marked nodes in source k's radius and in no other
    n_marked: int = None             # marked nodes
    n_covered: int = None            # marked nodes in at least one radius
    sources: np.ndarray = None       # int32 [K]: node id of source k
    direction: str = "dependents"
    max_hops: int = 0
    rounds: int = 0

    @property
    def k(self):
        return int(self.hist.shape[0])

    def members(self, k):
        """Node ids in source k's radius, ascending (the source itself is one of them)."""
        return np.flatnonzero((self.reach >> np.uint64(k)) & np.uint64(1)).tolist()

    def reached(self, k):
        return int(self.hist[k].sum())

    def reached_marked(self, k):
        return int(self.hist_marked[k].sum())

    def rollup(self, k, group_of):
        """group_of [N] (e.g. the service of each pod) -> [(group, count)] over k's radius, by count
        descending, then by group."""
        g = np.asarray(group_of)[np.asarray(self.members(k), np.int64)]
        groups, counts = np.unique(g, return_counts=True)
        out = [(x.item(), int(c)) for x, c in zip(groups, counts)]
        return sorted(out, key=lambda t: (-t[1], t[0]))

    def cover(self):
        """The greedy picks as (source slot, gain) pairs."""
        if self.order is None:
            return []
        return [(int(k), int(g)) for k, g in zip(self.order.tolist(), self.gain.tolist()) if k >= 0]

    def summary(self, names=None):
        """Plain ints and lists (the coordinator's additive key).  The source itself is not counted as
        its own dependent: `dependents` is the radius without it."""
        def name(i):
            return names[i] if names is not None else int(i)
        cands = []
        for k in range(self.k):
            s = int(self.sources[k])
            src_marked = int(self.hist_marked[k][0])
            anomalous = self.reached_marked(k) - src_marked
            c = {"component": name(s), "rank": k + 1, "dependents": self.reached(k) - 1,
                 "anomalous_dependents": anomalous, "depth": int(self.depth[k]),
                 "by_hop": self.hist[k].tolist(), "anomalous_by_hop": self.hist_marked[k].tolist()}
            if self.n_marked is not None:
                c["share_of_anomalous"] = self.reached_marked(k) / self.n_marked if self.n_marked else 0.0
                c["exclusive_anomalous"] = int(self.exclusive[k])
            cands.append(c)
        out = {"candidates": cands}
        if self.order is not None:
            cum, cov = 0, []
            for k, g in self.cover():
                cum += g
                cov.append({"component": name(int(self.sources[k])), "rank": k + 1, "gain": g,
                            "cumulative_share": cum / self.n_marked if self.n_marked else 0.0})
            out["cover"] = cov
            out["anomalous"] = int(self.n_marked)
            out["unreached"] = int(self.n_marked - self.n_covered)
        out["params"] = {"direction": self.direction, "max_hops": int(self.max_hops), "bins": int(self.hist.shape[1])}
        return out
