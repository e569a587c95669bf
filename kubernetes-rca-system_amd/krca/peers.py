"""Peer groups for krca_peer_score (include/krca.h): pods grouped by service (their
replicas), by node, and the nodes as one group.

``groups_from_labels`` turns one label per pod into the CSR the call reads; ``PeerGroups`` validates it
once on the host and keeps it on the engine's device; ``node_effects`` runs the node half of the chain
service -> node -> nodes-against-nodes (one step of a median polish): the group medians, by node, of the
pods' deviations from their replicas are the node effects, and one more call with all nodes as a single
group scores the nodes against each other.
"""
import numpy as np


def groups_from_labels(labels, n_groups=None):
    """labels int [P] (label < 0: the pod is in no group) -> (grp_ptr int64 [G + 1], member int32 [n]).
    G = n_groups or max(label) + 1; a group's members are in ascending pod order (stable)."""
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    keep = np.flatnonzero(lab >= 0)
    G = int(n_groups) if n_groups is not None else (int(lab[keep].max()) + 1 if len(keep) else 0)
    if len(keep) and int(lab[keep].max()) >= G:
        raise ValueError(f"label {int(lab[keep].max())} outside [0, {G})")
    order = keep[np.argsort(lab[keep], kind="stable")]
    grp_ptr = np.zeros(G + 1, np.int64)
    np.cumsum(np.bincount(lab[keep], minlength=G), out=grp_ptr[1:])
    return grp_ptr, order.astype(np.int32)


class PeerGroups:
    """The CSR of one grouping on the engine's device (``grp_ptr`` int64 [G + 1], ``member`` int32 [n]),
    validated once on the host: grp_ptr starts at 0, does not decrease and ends at len(member); every id
    is -1 (ignored by the call) or inside [0, n_pods); no pod is listed twice."""

    def __init__(self, engine, grp_ptr, member, n_pods):
        gp = np.ascontiguousarray(grp_ptr, np.int64).reshape(-1)
        mem = np.ascontiguousarray(member, np.int32).reshape(-1)
        if len(gp) < 1 or gp[0] != 0 or gp[-1] != len(mem) or (np.diff(gp) < 0).any():
            raise ValueError("grp_ptr must start at 0, not decrease and end at len(member)")
        if len(mem) and (mem.min() < -1 or mem.max() >= int(n_pods)):
            raise ValueError(f"member ids must be -1 or inside [0, {int(n_pods)})")
        listed = mem[mem >= 0]
        if len(np.unique(listed)) != len(listed):
            raise ValueError("a pod is listed more than once")
        self.n_pods, self.n_groups = int(n_pods), len(gp) - 1
        self.grp_ptr_host, self.member_host = gp, mem
        self.engine = engine
        self.grp_ptr = engine._dev(gp) if engine is not None and hasattr(engine, "_dev") else gp
        self.member = engine._dev(mem) if engine is not None and hasattr(engine, "_dev") else mem

    @classmethod
    def from_labels(cls, engine, labels, n_groups=None):
        gp, mem = groups_from_labels(labels, n_groups)
        return cls(engine, gp, mem, len(np.asarray(labels).reshape(-1)))

    def sizes(self):
        """Listed members per group (ids of -1 not counted), int64 [G]."""
        ok = np.concatenate([[0], np.cumsum(self.member_host >= 0)])
        return (ok[self.grp_ptr_host[1:]] - ok[self.grp_ptr_host[:-1]]).astype(np.int64)

    def group_of(self):
        """int32 [n_pods]: each pod's group, -1 for a pod in none."""
        g = np.full(self.n_pods, -1, np.int32)
        gid = np.repeat(np.arange(self.n_groups, dtype=np.int32), np.diff(self.grp_ptr_host))
        ok = self.member_host >= 0
        g[self.member_host[ok]] = gid[ok]
        return g

    def without(self, drop):
        """The same groups with the pods of the boolean mask drop [n_pods] left out (their ids become -1,
        which the call ignores)."""
        mem = self.member_host.copy()
        ok = mem >= 0
        mem[ok] = np.where(np.asarray(drop, bool)[mem[ok]], -1, mem[ok])
        return PeerGroups(self.engine, self.grp_ptr_host, mem, self.n_pods)


def node_effects(engine, peer, service_groups, node_groups, min_members=4, min_scale=0.0, out_thr=3.0):
    """Calls 2 and 3 of the chain.  peer: the pods' deviations from their replicas, [P, M] (the service
    call's "peer", device or host); service_groups: the PeerGroups of that call or None -- pods in no
    service group, or in one below min_members, carry a 0 that is no measurement and are left out of the
    node medians; node_groups: PeerGroups by node.
    -> dict: "effect" float32 [N, M] (per node the median over its pods of peer), "deviation" float32
    [N, M], "score" float32 [N] and "lead" int8 [N] (the nodes against the other nodes), "pods" int64 [N]
    (pods counted per node), "out" int32 [N, M] (pods of the node beyond out_thr), and the two calls' dicts
    under "by_node" / "nodes"."""
    groups = node_groups
    if service_groups is not None:
        size = service_groups.sizes()
        g = service_groups.group_of()
        groups = node_groups.without((g < 0) | (size[np.maximum(g, 0)] < int(min_members)))
    by_node = engine.peer_score(peer, groups, min_members=1, min_scale=min_scale, out_thr=out_thr)
    N = groups.n_groups
    every = (np.array([0, N], np.int64), np.arange(N, dtype=np.int32))
    nodes = engine.peer_score(by_node["grp_med"], every, min_members=min_members, min_scale=min_scale, out_thr=out_thr)
    return {"effect": by_node["grp_med_host"], "deviation": nodes["peer_host"], "score": nodes["score_host"],
            "lead": nodes["lead_host"], "pods": groups.sizes(), "out": by_node["grp_out_host"], "by_node": by_node,
            "nodes": nodes}
