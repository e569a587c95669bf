"""Structure of a dependency graph as the device computed it (include/krca.h g1, csrc/graph_struct.hip):
strongly connected components, the longest chain of the condensation and one witness cycle.

:class:`GraphStructure` holds the arrays of krca_graph_scc / krca_graph_chain / krca_graph_cycle as
host numpy arrays; its walkers are host code over those arrays (they need no GPU and are tested on
restated arrays).  ``NativeEngine.graph_structure`` builds it.
"""
from dataclasses import dataclass, field

import numpy as np

F_CYCLIC, F_SELF_LOOP, F_REP = 1, 2, 4  # bits of GraphStructure.flags


@dataclass
class GraphStructure:
    n: int
    comp: np.ndarray                 # int32 [N]: the smallest node id of the node's component
    flags: np.ndarray                # uint8 [N]: F_CYCLIC | F_SELF_LOOP | F_REP
    n_components: int = 0
    n_cyclic: int = 0                # cyclic components (>= 2 nodes, or a self-loop)
    n_cyclic_nodes: int = 0
    largest_size: int = 0
    first_cyclic_label: int = -1
    n_bad_edges: int = 0             # col entries outside [0, N): no edges
    depth_dn: np.ndarray = None      # int32 [N] (chain=True): components on the longest chain forward
    depth_up: np.ndarray = None      # int32 [N]: the same backward
    next: np.ndarray = None          # int32 [N]: label of the next component on that chain, -1 at a sink
    longest: int = None              # max depth_dn: exact on an acyclic graph, a lower bound otherwise
    start: int = None                # the smallest label that attains it
    root: int = -1                   # cycle=True and a cyclic component exists: first_cyclic_label
    hop: np.ndarray = None           # int32 [N]: next node on a shortest path to root (hop[root] closes the cycle)
    rounds: dict = field(default_factory=dict)  # device rounds per phase

    def cyclic_groups(self):
        """Labels of the cyclic components, ascending."""
        f = self.flags
        return np.flatnonzero((f & F_CYCLIC != 0) & (f & F_REP != 0)).astype(np.int64).tolist()

    def members(self, label):
        """Node ids of component `label`, ascending."""
        return np.flatnonzero(self.comp == label).tolist()

    def longest_chain(self):
        """Component labels from `start` following `next`: `longest` labels ([] without chain data)."""
        if self.next is None or self.start is None or self.start < 0:
            return []
        out, v = [], int(self.start)
        while v >= 0:
            out.append(v)
            if len(out) > self.n:
                raise ValueError("graph structure: `next` does not end at a sink")
            v = int(self.next[v])
        return out

    def first_cycle(self):
        """Node list of the witness cycle, starting at the root (a self-loop: [root]); None when the
        graph is acyclic or no cycle was requested."""
        if self.hop is None or self.root < 0 or int(self.hop[self.root]) < 0:
            return None
        out, v = [int(self.root)], int(self.hop[self.root])
        while v != self.root:
            if v < 0 or len(out) > self.n:
                raise ValueError("graph structure: `hop` does not lead back to the root")
            out.append(v)
            v = int(self.hop[v])
        return out

    def summary(self):
        """Plain ints and lists (the agents' additive key)."""
        out = {"nodes": int(self.n), "components": int(self.n_components), "cyclic_groups": int(self.n_cyclic),
               "cyclic_nodes": int(self.n_cyclic_nodes), "largest_group": int(self.largest_size),
               "bad_edges": int(self.n_bad_edges), "cyclic_group_labels": self.cyclic_groups()}
        if self.next is not None:
            out["longest_chain"] = int(self.longest)
            out["longest_chain_exact"] = self.n_cyclic == 0
            out["chain"] = self.longest_chain()
        if self.hop is not None:
            out["cycle"] = self.first_cycle()
        return out


def rotate_to_lowest(cycle):
    """The cycle rotated to start at its lowest id (as tracecols.first_cycle reports it)."""
    if not cycle:
        return cycle
    k = cycle.index(min(cycle))
    return cycle[k:] + cycle[:k]


def out_csr(n, src, dst):
    """Out-edge CSR (row u = successors of u, pull = 0) from an edge list; int64 row_ptr, int32 col."""
    src = np.asarray(src, np.int64).reshape(-1)
    dst = np.asarray(dst, np.int64).reshape(-1)
    order = np.argsort(src, kind="stable")
    row_ptr = np.zeros(n + 1, np.int64)
    if len(src):
        np.cumsum(np.bincount(src, minlength=n), out=row_ptr[1:])
    return row_ptr, dst[order].astype(np.int32)
