"""Host helpers for the lead/lag correlation along dependency edges (krca_corr_edges; DESIGN.md
§3.14): decoding of dep_best, the edge it came from, and the text form of a follower record."""
import numpy as np

ID_BASE = 0x7FFFFFFF  # dep_best's low word is ID_BASE - dependency id, so the max prefers the lower id


def encode_dep_best(r, dep):
    """The dep_best word of a DEP_LEADS edge with correlation r (float32) towards dependency `dep`."""
    bits = int(np.abs(np.float32(r)).view(np.uint32))
    return (bits << 32) | (ID_BASE - int(dep))


def decode_dep_best(v):
    """dep_best value -> (dependency id, |r| as float, |r|'s float32 bits), or None (0: no leading
    dependency)."""
    v = int(v)
    if v <= 0:
        return None
    bits = v >> 32
    return ID_BASE - (v & 0xFFFFFFFF), float(np.uint32(bits).view(np.float32)), bits


def edge_of(row_ptr, col, lag, r_lag, caller, dep, r_bits=None):
    """CSR position of the edge caller -> dep (row dep of the pull-CSR) that dep_best[caller] came
    from: among duplicates, the first with a positive lag whose |r_lag| has the bits r_bits."""
    e0, e1 = int(row_ptr[dep]), int(row_ptr[dep + 1])
    hits = e0 + np.flatnonzero(np.asarray(col[e0:e1]) == caller)
    if r_bits is not None:
        mag = np.abs(np.asarray(r_lag)[hits].astype(np.float32)).view(np.uint32)
        hits = hits[(mag == np.uint32(r_bits)) & (np.asarray(lag)[hits] > 0)]
    if len(hits) == 0:
        raise ValueError(f"no edge {caller} -> {dep} matches dep_best")
    return int(hits[0])


def follower(name, dep_name, lag_steps, r):
    """One follower record (plain Python values) of the Coordinator's `correlations` key."""
    return {"component": f"Pod/{name}", "follows": f"Pod/{dep_name}", "lag_steps": int(lag_steps), "r": float(r)}


def describe(f):
    """'Pod/a follows Pod/b by 4 steps (r = 0.83)' (a follower record)."""
    n = int(f["lag_steps"])
    return f"{f['component']} follows {f['follows']} by {n} step{'s' if n != 1 else ''} (r = {f['r']:.2f})"
