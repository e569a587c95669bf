"""MetricsAgent: per-pod usage thresholds (+ rolling z-score anomalies on the bulk path).

Reference: ref:agents/metrics_agent.py:4-365.  The per-pod threshold scans
(``_analyze_cpu_usage`` :69-114, ``_analyze_memory_usage`` :116-161) are the hot loops; here
they are one device pass (``krca_usage_flags`` / ``krca_rolling_score``) and the host only
formats the findings for the flagged pods, in pod order, with the reference's strings.

Node pressure (:163-209), resource configuration (:211-277) and HPA checks (:279-365) are
dict walks over a handful of objects and stay on the host.

Bulk path (additive): when the client exposes
``get_pod_metric_tensor(namespace) -> (pod_names, x)`` with ``x`` a float32 device tensor laid
out ``[T][P][M]`` (time-major; channel 0 = CPU %, channel 1 = memory %), the thresholds read the
last sample and the rolling z-score kernel adds the ``anomalies`` key (schema of
ref:agent_coordinator.py:113-115: resource / description / severity / deviation).
"""
import numpy as np

from .base import BaseAgent

CPU_CH, MEM_CH = 0, 1
# peer deviation defaults per peer_value: (scale floor, pod threshold), and the node threshold.  Each
# threshold is 4 % above the largest null maximum measured on clean synth.make_metrics_replicas data at C2
# size with the NumPy restatement (the table of DESIGN.md §3.20)
PEER_DEFAULTS = {"shift": (0.5, 6.5), "level": (1.0, 7.6)}
NODE_THRESHOLD = 7.0
# flag bits produced by the device kernels (include/krca.h)
F_CPU80, F_CPU90, F_MEM80, F_MEM90 = 1, 2, 4, 8


def to_f32_threshold_safe(values):
    """float64 -> float32 such that every ``> 80`` and ``> 90`` test keeps its float64 answer.

    Rounding to nearest is monotone and 80/90 are exact in float32, so the only flip is a
    value just above a threshold rounding down onto it; such values are nudged one ulp up.
    """
    v = np.asarray(values, dtype=np.float64)
    f = v.astype(np.float32)
    for t in (80.0, 90.0):
        bump = (v > t) & (f <= np.float32(t))
        f[bump] = np.nextafter(np.float32(t), np.float32(np.inf))
    return f


class MetricsAgent(BaseAgent):
    def __init__(self, k8s_client, engine=None, window=60, z_threshold=3.0, anomaly_topk=10, timeline=False,
                 timeline_gap=3, timeline_min_count=3, level_shift=False, shift_baseline=120, shift_recent=3,
                 shift_guard=0, shift_min_scale=0.0, shift_threshold=None, peer_deviation=False, peer_value="shift",
                 peer_min_members=4, peer_min_scale=None, peer_threshold=None, node_threshold=None):
        super().__init__(k8s_client, engine)
        self.window = window
        self.z_threshold = z_threshold
        self.anomaly_topk = anomaly_topk
        # timeline=True: the bulk path scores with krca_rolling_timeline (same pass, same scores) and
        # the result gains the additive key "anomaly_timeline": when each reported anomaly began
        self.timeline = bool(timeline)
        self.timeline_gap = timeline_gap
        self.timeline_min_count = timeline_min_count
        # level_shift=True: the bulk path also runs krca_shift_score (the median of the last shift_recent
        # samples against the median / MAD of the shift_baseline samples before them and a guard) and the
        # result gains the additive key "level_shifts": the sustained changes of level, which the
        # last-step z-score above cannot see
        self.level_shift = bool(level_shift)
        self.shift_baseline = int(shift_baseline)
        self.shift_recent = int(shift_recent)
        self.shift_guard = int(shift_guard)
        self.shift_min_scale = float(shift_min_scale)
        self.shift_threshold = shift_threshold  # None: max(z_threshold, rca.null_floor(P*M))
        self.last_scores = None  # device outputs of the last bulk run (used by the Coordinator)
        self.last_shift = None   # outputs of the last krca_shift_score run (level_shift=True)
        # peer_deviation=True: the bulk path also scores each pod against its replicas now, not against its
        # own past (krca_peer_score over the shift statistics, grouped by the client's get_pod_groups
        # labels), then the nodes against each other; the result gains the additive keys
        # "peer_deviations", "service_wide" and "node_deviations" 
        if peer_value not in PEER_DEFAULTS:
            raise ValueError(f"peer_value must be one of {sorted(PEER_DEFAULTS)}")
        self.peer_deviation = bool(peer_deviation)
        self.peer_value = peer_value
        self.peer_min_members = int(peer_min_members)
        self.peer_min_scale = peer_min_scale    # None: PEER_DEFAULTS[peer_value][0]
        self.peer_threshold = peer_threshold    # None: PEER_DEFAULTS[peer_value][1]
        self.node_threshold = node_threshold    # None: NODE_THRESHOLD
        self.last_peer = None    # outputs of the last peer-deviation run (peer_deviation=True)

    # ------------------------------------------------------------------------------------
    def analyze(self, namespace, context=None, **kwargs):
        self.reset()
        self.last_scores = None
        self.last_shift = None
        self.last_peer = None
        try:
            self._maybe_set_context(context)
            bulk = getattr(self.k8s_client, "get_pod_metric_tensor", None)
            anomalies = timeline = shifts = peers = None
            if bulk is not None:
                names, x = bulk(namespace)
                pods, flags, anomalies = self._score_tensor(names, x)
                if self.timeline and self.last_scores is not None:
                    timeline = self._anomaly_timeline(names, anomalies, self.last_scores)
                if self.level_shift:
                    shifts = self._level_shifts(names, x)
                if self.peer_deviation:
                    peers = self._peer_deviations(namespace, names, x)
            else:
                pod_metrics = self.k8s_client.get_pod_metrics(namespace)
                pods, flags = self._score_dict(pod_metrics)
            node_metrics = self.k8s_client.get_node_metrics()
            self._report_usage(pods, flags, "CPU", "cpu", CPU_CH, F_CPU80, F_CPU90)
            self._report_usage(pods, flags, "memory", "memory", MEM_CH, F_MEM80, F_MEM90)
            self._analyze_node_resources(node_metrics)
            self._analyze_resource_configurations(namespace)
            self._analyze_hpa_configurations(namespace)
            res = self.get_results()
            if anomalies is not None:
                res["anomalies"] = anomalies
            if timeline is not None:
                res["anomaly_timeline"] = timeline
            if shifts is not None:
                res["level_shifts"] = shifts
            if peers is not None:
                res.update(peers)
            return res
        except Exception as e:  # ref:agents/metrics_agent.py:58-67
            return self._error_result("metrics", e)

    # -- dict path (C1): usage_percentage per pod ----------------------------------------
    def _score_dict(self, pod_metrics):
        names = list(pod_metrics.keys())
        if not names:
            return [], None
        raw = np.zeros((len(names), 2), dtype=np.float64)
        for i, n in enumerate(names):
            m = pod_metrics[n]
            raw[i, 0] = m.get("cpu", {}).get("usage_percentage", 0)
            raw[i, 1] = m.get("memory", {}).get("usage_percentage", 0)
        usage = to_f32_threshold_safe(raw)
        flags = self.engine.usage_flags(usage)
        # evidence is printed from the caller's own values, exactly as the reference does
        pods = [(n,
                 pod_metrics[n].get("cpu", {}).get("usage_percentage", 0),
                 pod_metrics[n].get("memory", {}).get("usage_percentage", 0)) for n in names]
        return pods, flags

    # -- bulk path (C2-C5): [T][P][M] float32 device tensor ------------------------------
    def _score_tensor(self, names, x):
        T, P, M = x.shape
        if P == 0:
            return [], None, []
        if self.timeline:
            out = self.engine.rolling_timeline(x, window=self.window, z_threshold=self.z_threshold,
                                               gap=self.timeline_gap, min_count=self.timeline_min_count)
        else:
            out = self.engine.rolling_score(x, window=self.window, z_threshold=self.z_threshold)
        self.last_scores = out
        flags = out["flags"]
        flagged = np.nonzero(flags & (F_CPU80 | F_MEM80))[0]
        last = self.engine.gather_last(x, flagged)  # [n_flagged, M] float32 host copy
        lut = {int(p): last[i] for i, p in enumerate(flagged)}
        pods = _LazyPods(names, lut)
        anomalies = []
        k = min(self.anomaly_topk, P)
        idx, val = self.engine.topk(out["score"], k)
        for p, s in zip(idx.tolist(), val.tolist()):
            if not s > self.z_threshold:
                break
            anomalies.append({
                "resource": f"Pod/{names[p]}",
                "description": (f"Rolling z-score {s:.2f} over a {self.window}-step window; "
                                f"{int(out['n_exceed_host'][p])} samples beyond |z|>{self.z_threshold:g}"),
                "severity": "high" if s > 2 * self.z_threshold else "medium",
                "deviation": float(s),
            })
        return pods, flags, anomalies

    def _anomaly_timeline(self, names, anomalies, out):
        """Per reported anomaly, in the order of `anomalies`: onset step, last step, episode count,
        lead metric and number of metrics involved (onset_step -1: the pod is anomalous at the last
        step but has no sustained episode)."""
        index = {f"Pod/{n}": p for p, n in enumerate(names)} if anomalies else {}
        rows = []
        for a in anomalies:
            p = index[a["resource"]]
            rows.append({"resource": a["resource"], "onset_step": int(out["onset_host"][p]),
                         "last_step": int(out["last_host"][p]), "episode_count": int(out["count_host"][p]),
                         "lead_metric": int(out["lead_host"][p]), "n_metrics": int(out["n_metrics_host"][p])})
        return rows

    def _level_shifts(self, names, x):
        """The top anomaly_topk pods by level-shift score above the threshold, in rank order: the lead
        metric's signed shift with its baseline median, recent median and scale."""
        T, P, M = x.shape
        B, R, G = self.shift_baseline, self.shift_recent, self.shift_guard
        if P == 0:
            return []
        if T < B + G + R:
            self.add_reasoning_step(
                observation=f"Metric history of {T} steps is shorter than the level-shift windows "
                            f"({B} baseline + {G} guard + {R} recent)",
                conclusion="Unable to score level shifts")
            return []
        from krca.rca import null_floor
        out = self.engine.shift_score(x, baseline=B, recent=R, guard=G, min_scale=self.shift_min_scale)
        self.last_shift = out
        thr = (float(self.shift_threshold) if self.shift_threshold is not None
               else max(float(self.z_threshold), null_floor(P * M)))
        rows = []
        idx, val = self.engine.topk(out["score"], min(self.anomaly_topk, P))
        for p, s in zip(idx.tolist(), val.tolist()):
            if not s > thr:
                break
            m = int(out["lead_host"][p])
            med, mad, rec = (float(out[k][p, m]) for k in ("base_med_host", "base_mad_host", "recent_med_host"))
            den, floor = 1.4826 * mad, float(np.float32(self.shift_min_scale))  # krca_shift_score's scale
            if not den > floor:
                den = floor
            rows.append({
                "resource": f"Pod/{names[p]}",
                "metric": m,
                "shift": float(out["shift_host"][p, m]),
                "baseline": med,
                "recent": rec,
                "scale": float(den),
                "description": (f"Level shift of {float(out['shift_host'][p, m]):+.2f} robust deviations in metric {m}: "
                                f"median {rec:.2f} over the last {R} steps against {med:.2f} over the "
                                f"{B} steps before them"),
                "severity": "high" if s > 2 * thr else "medium",
            })
        return rows

    def _peer_deviations(self, namespace, names, x):
        """{"peer_deviations", "service_wide", "node_deviations"}: the top anomaly_topk pods whose deviation
        from their replicas exceeds the threshold, in rank order; the services whose own median shift exceeds
        the level-shift threshold (the whole service moved, not a pod); the nodes whose pods deviate from
        their replicas together, against the other nodes."""
        from krca.peers import PeerGroups, node_effects
        from krca.rca import null_floor
        res = {"peer_deviations": [], "service_wide": [], "node_deviations": []}
        T, P, M = x.shape
        B, R, G = self.shift_baseline, self.shift_recent, self.shift_guard
        if P == 0:
            return res
        getter = getattr(self.k8s_client, "get_pod_groups", None)
        labels = (getter(namespace) or {}) if getter is not None else {}
        if labels.get("service") is None:
            self.add_reasoning_step(
                observation="The client serves no service labels for its pods (get_pod_groups)",
                conclusion="Unable to score peer deviations")
            return res
        if T < B + G + R:
            self.add_reasoning_step(
                observation=f"Metric history of {T} steps is shorter than the level-shift windows "
                            f"({B} baseline + {G} guard + {R} recent)",
                conclusion="Unable to score peer deviations")
            return res
        sh = self.last_shift
        if sh is None:
            sh = self.engine.shift_score(x, baseline=B, recent=R, guard=G, min_scale=self.shift_min_scale)
        floor, thr = PEER_DEFAULTS[self.peer_value]
        floor = float(floor if self.peer_min_scale is None else self.peer_min_scale)
        thr = float(thr if self.peer_threshold is None else self.peer_threshold)
        node_thr = float(NODE_THRESHOLD if self.node_threshold is None else self.node_threshold)
        shift_thr = (float(self.shift_threshold) if self.shift_threshold is not None
                     else max(float(self.z_threshold), null_floor(P * M)))
        services = PeerGroups.from_labels(self.engine, labels["service"])
        args = dict(min_members=self.peer_min_members, min_scale=floor, out_thr=thr)
        out = self.engine.peer_score(sh["shift" if self.peer_value == "shift" else "recent_med"], services, **args)
        own = out if self.peer_value == "shift" else self.engine.peer_score(sh["shift"], services, **args)
        self.last_peer = {"value": self.peer_value, "shift": sh, "service": out, "service_shift": own, "nodes": None,
                          "min_scale": floor, "threshold": thr, "node_threshold": node_thr}
        group_of, size = services.group_of(), services.sizes()
        idx, val = self.engine.topk(out["score"], min(self.anomaly_topk, P))
        for p, s in zip(idx.tolist(), val.tolist()):
            if not s > thr:
                break
            m, g = int(out["lead_host"][p]), int(group_of[p])
            med, mad = float(out["grp_med_host"][g, m]), float(out["grp_mad_host"][g, m])
            dev = float(out["peer_host"][p, m])
            den = 1.4826 * mad
            if not den > float(np.float32(floor)):
                den = float(np.float32(floor))
            others = int(out["grp_out_host"][g, m]) - 1
            res["peer_deviations"].append({
                "resource": f"Pod/{names[p]}",
                "service": g,
                "metric": m,
                "deviation": dev,
                "group_median": med,
                "scale": float(den),
                "peers_out": others,
                "group_size": int(size[g]),
                "description": (f"Metric {m} deviates {dev:+.2f} robust deviations from the {int(size[g]) - 1} other "
                                f"replicas of service group {g} ({others} of them are out as well)"),
                "severity": "high" if s > 2 * thr else "medium",
            })
        gm = np.where(np.isnan(own["grp_med_host"]), np.float32(0), np.abs(own["grp_med_host"]))
        moved = gm.max(axis=1) if gm.shape[0] else np.zeros(0, np.float32)
        for g in sorted(np.flatnonzero((moved > shift_thr) & (size >= self.peer_min_members)).tolist(),
                        key=lambda g: (-float(moved[g]), g)):
            m = int(gm[g].argmax())
            res["service_wide"].append({
                "service": g,
                "metric": m,
                "shift": float(own["grp_med_host"][g, m]),
                "members": int(size[g]),
                "description": (f"The whole of service group {g} moved: the median level shift of its {int(size[g])} "
                                f"replicas in metric {m} is {float(own['grp_med_host'][g, m]):+.2f} robust deviations"),
            })
        if labels.get("node") is not None:
            nodes = PeerGroups.from_labels(self.engine, labels["node"])
            ne = node_effects(self.engine, out["peer"], services, nodes, min_members=self.peer_min_members, out_thr=thr)
            self.last_peer["nodes"] = ne
            order = sorted(range(nodes.n_groups), key=lambda n: (-float(ne["score"][n]), n))[:self.anomaly_topk]
            for n in order:
                s = float(ne["score"][n])
                if not s > node_thr:
                    break
                m = int(ne["lead"][n])
                res["node_deviations"].append({
                    "node": n,
                    "metric": m,
                    "deviation": float(ne["deviation"][n, m]),
                    "effect": float(ne["effect"][n, m]),
                    "pods": int(ne["pods"][n]),
                    "description": (f"The {int(ne['pods'][n])} pods of node {n} deviate from their replicas together: "
                                    f"metric {m} by a median of {float(ne['effect'][n, m]):+.2f}, "
                                    f"{float(ne['deviation'][n, m]):+.2f} robust deviations from the other nodes"),
                    "severity": "high" if s > 2 * node_thr else "medium",
                })
        return res

    # -- shared reporting (ref:agents/metrics_agent.py:69-161) ---------------------------
    def _report_usage(self, pods, flags, label, key, ch, f80, f90):
        if not len(pods):
            self.add_reasoning_step(observation=f"No {label} metrics data available",
                                    conclusion=f"Unable to analyze {label} usage")
            return
        self.add_reasoning_step(observation=f"Analyzing {label} usage for {len(pods)} pods",
                                conclusion=f"Beginning {label} usage analysis")
        hit = np.nonzero(flags & f80)[0]
        if len(hit):
            sel = [pods[int(i)] for i in hit]
            vals = [(p[0], p[1 + ch]) for p in sel]
            pod_list = ", ".join(f"{name} ({usage:.1f}%)" for name, usage in vals)
            severe = bool(np.any(flags[hit] & f90))
            if ch == CPU_CH:
                self.add_finding(
                    component="Pods CPU Usage",
                    issue=f"High CPU usage detected in {len(vals)} pods",
                    severity="high" if severe else "medium",
                    evidence=f"Pods with high CPU usage: {pod_list}",
                    recommendation="Consider scaling these deployments or optimizing the application code")
                self.add_reasoning_step(
                    observation=f"Detected {len(vals)} pods with CPU usage above 80%",
                    conclusion="High CPU usage may indicate resource constraints or inefficient application code")
            else:
                self.add_finding(
                    component="Pods Memory Usage",
                    issue=f"High memory usage detected in {len(vals)} pods",
                    severity="high" if severe else "medium",
                    evidence=f"Pods with high memory usage: {pod_list}",
                    recommendation="Consider increasing memory limits, scaling horizontally, or investigating memory leaks")
                self.add_reasoning_step(
                    observation=f"Detected {len(vals)} pods with memory usage above 80%",
                    conclusion="High memory usage may indicate memory leaks or insufficient resource allocation")
        else:
            self.add_reasoning_step(observation=f"No pods with high {label} usage detected",
                                    conclusion=f"{label[0].upper() + label[1:]} usage appears to be within acceptable limits")

    # -- node pressure: 3 nodes in C1, host (ref:agents/metrics_agent.py:163-209) --------
    def _analyze_node_resources(self, node_metrics):
        if not node_metrics:
            self.add_reasoning_step(observation="No node metrics data available",
                                    conclusion="Unable to analyze node resource usage")
            return
        self.add_reasoning_step(observation=f"Analyzing resource usage for {len(node_metrics)} nodes",
                                conclusion="Beginning node resource analysis")
        pressured = []
        for node, m in node_metrics.items():
            c = m.get("cpu", {}).get("usage_percentage", 0)
            mem = m.get("memory", {}).get("usage_percentage", 0)
            if c > 80 or mem > 80:
                pressured.append((node, c, mem))
        if not pressured:
            self.add_reasoning_step(observation="No nodes with high resource pressure detected",
                                    conclusion="Node resource usage appears to be within acceptable limits")
            return
        listing = ", ".join(f"{n} (CPU: {c:.1f}%, Memory: {mem:.1f}%)" for n, c, mem in pressured)
        self.add_finding(
            component="Node Resources",
            issue=f"Resource pressure detected on {len(pressured)} nodes",
            severity="high" if any(c > 90 or mem > 90 for _, c, mem in pressured) else "medium",
            evidence=f"Nodes under resource pressure: {listing}",
            recommendation="Consider adding more nodes to the cluster or optimizing workload distribution")
        self.add_reasoning_step(
            observation=f"Detected {len(pressured)} nodes with high resource usage",
            conclusion="Node resource pressure may be affecting overall cluster performance and pod scheduling")

    # -- requests/limits (ref:agents/metrics_agent.py:211-277) ---------------------------
    def _analyze_resource_configurations(self, namespace):
        try:
            deployments = self.k8s_client.get_deployments(namespace)
            if not deployments:
                self.add_reasoning_step(observation=f"No deployments found in namespace {namespace}",
                                        conclusion="Unable to analyze resource configurations")
                return
            self.add_reasoning_step(
                observation=f"Analyzing resource configurations for {len(deployments)} deployments",
                conclusion="Beginning resource configuration analysis")
            missing = []
            for d in deployments:
                dname = d["metadata"]["name"]
                for c in d["spec"]["template"]["spec"]["containers"]:
                    res = c.get("resources", {})
                    req, lim = ("requests" in res), ("limits" in res)
                    complete = (req and "cpu" in res["requests"] and "memory" in res["requests"]
                                and lim and "cpu" in res["limits"] and "memory" in res["limits"])
                    if not complete:
                        missing.append(f"{dname}/{c['name']}")
            if missing:
                self.add_finding(
                    component="Resource Configuration",
                    issue=f"Missing resource requests or limits in {len(missing)} containers",
                    severity="medium",
                    evidence=f"Containers with missing resource configurations: {', '.join(missing)}",
                    recommendation="Add appropriate CPU and memory requests and limits to all containers")
                self.add_reasoning_step(
                    observation=f"Detected {len(missing)} containers with missing resource configurations",
                    conclusion="Missing resource configurations can lead to resource contention and unpredictable behavior")
            else:
                self.add_reasoning_step(observation="All containers have resource requests and limits configured",
                                        conclusion="Resource configurations appear to be properly defined")
        except Exception as e:
            self.add_reasoning_step(observation=f"Error analyzing resource configurations: {str(e)}",
                                    conclusion="Unable to complete resource configuration analysis")

    # -- HPA (ref:agents/metrics_agent.py:279-365) ---------------------------------------
    _HPA_FINDINGS = {
        "at_max_capacity": ("HPA is at maximum capacity ({cur}/{mx} replicas)", "high",
                            "HPA {name} is running at maximum capacity of {mx} replicas",
                            "Consider increasing the maximum replicas for this HPA"),
        "narrow_range": ("HPA has a narrow scaling range ({mn}-{mx} replicas)", "low",
                         "HPA {name} has min={mn}, max={mx} replicas",
                         "Consider widening the scaling range to allow more flexibility"),
        "scaling_delay": ("HPA desired replicas not matching current replicas", "medium",
                          "HPA {name} has desired replicas > current replicas",
                          "Investigate potential issues preventing scaling or configure less aggressive scaling"),
    }

    def _analyze_hpa_configurations(self, namespace):
        try:
            hpas = self.k8s_client.get_hpas(namespace)
            if not hpas:
                self.add_reasoning_step(observation=f"No HPAs found in namespace {namespace}",
                                        conclusion="No autoscaling configurations to analyze")
                return
            self.add_reasoning_step(observation=f"Analyzing {len(hpas)} Horizontal Pod Autoscalers",
                                    conclusion="Beginning HPA configuration analysis")
            problems = []
            for h in hpas:
                name = h["metadata"]["name"]
                mn = h["spec"].get("minReplicas", 1)
                mx = h["spec"].get("maxReplicas", 1)
                cur = h["status"].get("currentReplicas", 0)
                want = h["status"].get("desiredReplicas", 0)
                if cur == mx and cur > 0:
                    problems.append(("at_max_capacity", name, mn, mx, cur))
                if mx - mn < 2 and mn > 1:
                    problems.append(("narrow_range", name, mn, mx, cur))
                if want > cur:
                    problems.append(("scaling_delay", name, mn, mx, cur))
            if problems:
                for kind, name, mn, mx, cur in problems:
                    issue, sev, ev, rec = self._HPA_FINDINGS[kind]
                    fmt = dict(name=name, mn=mn, mx=mx, cur=cur)
                    self.add_finding(component=f"HPA/{name}", issue=issue.format(**fmt), severity=sev,
                                     evidence=ev.format(**fmt), recommendation=rec)
                self.add_reasoning_step(
                    observation=f"Detected {len(problems)} HPAs with potential configuration issues",
                    conclusion="HPA configuration issues may be affecting the ability to scale effectively")
            else:
                self.add_reasoning_step(observation="All HPAs appear to be properly configured",
                                        conclusion="HPA configurations look appropriate for the current workload")
        except Exception as e:
            self.add_reasoning_step(observation=f"Error analyzing HPA configurations: {str(e)}",
                                    conclusion="Unable to complete HPA configuration analysis")


class _LazyPods:
    """Sequence view over a million-pod tensor: only flagged rows are ever materialised."""

    def __init__(self, names, last_by_pod):
        self.names = names
        self.last = last_by_pod

    def __len__(self):
        return len(self.names)

    def __getitem__(self, p):
        row = self.last[p]
        return (self.names[p], float(row[CPU_CH]), float(row[MEM_CH]))
