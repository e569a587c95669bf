"""Host helpers for the anomaly timeline (krca_rolling_timeline / krca_rca_precede):
decoding of dep_first and the text form of a timeline entry."""

NO_DEP = (1 << 63) - 1  # dep_first of a pod without an earlier dependency (INT64_MAX)


def decode_dep_first(v):
    """dep_first value -> (onset step, pod id) of the earliest earlier dependency, or None."""
    v = int(v)
    if v == NO_DEP or v < 0:
        return None
    return v >> 32, v & 0xFFFFFFFF


def entry(name, onset, last, count, lead, n_metrics, peak=None):
    """One pod's timeline record (plain Python values), or None for a pod without a kept episode."""
    if int(onset) < 0:
        return None
    e = {"resource": f"Pod/{name}", "onset_step": int(onset), "last_step": int(last), "episode_count": int(count),
         "lead_metric": int(lead), "n_metrics": int(n_metrics)}
    if peak is not None:
        e["peak"] = float(peak)
    return e


def format_entry(e, n_steps=None, metric_names=None):
    """'Pod/x: anomalous from step 1380 (60 steps before the end) to 1439, 57 samples beyond the
    threshold on 3 metrics, metric 2 first'."""
    m = e["lead_metric"]
    lead = metric_names[m] if metric_names is not None and 0 <= m < len(metric_names) else f"metric {m}"
    ago = f" ({int(n_steps) - 1 - e['onset_step']} steps before the end)" if n_steps is not None else ""
    s = (f"{e['resource']}: anomalous from step {e['onset_step']}{ago} to {e['last_step']}, "
         f"{e['episode_count']} samples beyond the threshold on {e['n_metrics']} "
         f"metric{'s' if e['n_metrics'] != 1 else ''}, {lead} first")
    if "peak" in e:
        s += f", peak |z| {e['peak']:.2f}"
    return s


def format_follower(name, dep_name, lead_steps):
    """'Pod/a followed Pod/b by 12 steps' (a first_movers(..., explain=) record)."""
    return f"Pod/{name} followed Pod/{dep_name} by {int(lead_steps)} steps"
